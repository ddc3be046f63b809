"""The yardstick of the n-gram mixture's ranking, prediction and completion tests (tests/test_ngram_mix_cpu.py, tests/test_gpu_rank_ngram.py,
tests/test_gpu_complete_ngram.py): the oracle LM's float64 logits, ``jlm_amd.ngram.mixed_logits`` over them, the definition of
jlm_rank_rows on the result (tests/rank_cases.py) and the beam of ``jlm_amd.complete.merge_reference``'s key followed on the device's
own parents (tests/test_gpu_complete.py oracle_follow, with the mixed logits in the plain ones' place).

The table is counted from the ranked stream itself (``estimate``), with lam = 0.5, so that it matters: ``moved_share`` is the share of
positions whose exact mixed rank differs from the plain one, and the tests assert at least a tenth for every model -- no test passes
by ignoring the table.
"""
import numpy as np

from jlm_amd.ngram import NGramMix, NGramTable, estimate, mixed_logits, pack
from tests import rank_cases as rc
from tests.ngram_mix_budget import row_bar

EOS = 1
LAM = 0.5
CUTS = ([45], [20, 20, 5], [7, 38])
MAX_PREFIX = 3
TOK_ATOL = 1e-5            # tests/test_gpu_score.py's bar on a word's nll
TOL_E2E = 1e-4             # tests/test_gpu_complete.py: a cut of the beam closer than this is ambiguous


def stream(V, B=3, n=45, seed=11):
    """B streams of n steps over a pool of a dozen words (tests/test_gpu_cache.py _stream): bigrams and trigrams repeat"""
    rng = np.random.RandomState(seed)
    pool = rng.randint(2, V, size=12)
    s = pool[rng.randint(0, 12, size=(B, n + 1))].astype(np.int32)
    return s[:, :-1], s[:, 1:]


def stream_table(x, y, V, order, lam=LAM):
    """the NGramMix counted from the streams themselves: every row a sentence"""
    ids = []
    for b in range(x.shape[0]):
        ids += [int(x[b, 0])] + [int(w) for w in y[b]] + [EOS]
    return NGramMix(estimate(np.array(ids), V, order), lam)


def leaky_table(mix, V):
    """``mix``'s table with the n-grams of every fifth word dropped, as a file read with a smaller vocabulary drops them: it no longer
    sums to one"""
    t = mix.table
    keep = np.ones(len(t), dtype=bool)
    for sh in (0, 21, 42):
        w = ((t.keys >> sh) & 0x1FFFFF) - 1
        keep &= ~((w >= 0) & (w % 5 == 3))
    return NGramMix(NGramTable(t.keys[keep], t.lp[keep], t.bow[keep], t.order), mix.lam)


def hist_of(words):
    """(u, v): the last two of a list of word ids, -1 where there is none"""
    w = [int(a) for a in words][-2:]
    return [-1] * (2 - len(w)) + w


def back_of(table, hist):
    """bow(u v) + bow(v) of the contexts the table's order uses of a history (what tests/ngram_mix_budget.py calls back)"""
    h = list(table.context([a for a in hist if a >= 0]))
    return sum((table.entry(h[i:]) or (0.0, 0.0))[1] for i in range(len(h)))


def oracle_run(lm, x):
    """y [B, n, V] float64: the oracle's logits of every step of streams from the zero state"""
    B, n = x.shape
    h, c = lm.zero_state(B)
    ys = []
    for t in range(n):
        h, c = lm.lstm_cell(x[:, t], h, c)
        ys.append(np.array(lm.project(h), dtype=np.float64))
    return np.stack(ys, axis=1)


def oracle_mixed(ys, x, mix, self_norm, tail=None):
    """-> (ymix [B, n, V]: mixed_logits over the oracle's logits with the history (x[t - 1], x[t]) -- tail[b][1] before x[b, 0] --,
    bars [B, n]: tests/ngram_mix_budget.py's row bar of every position)"""
    B, n, V = ys.shape
    ymix, bars = np.empty_like(ys), np.zeros((B, n))
    for b in range(B):
        for t in range(n):
            h = hist_of(([int(tail[b][1])] if tail is not None and t == 0 else []) + [int(a) for a in x[b, max(t - 1, 0):t + 1]])
            ymix[b, t] = mixed_logits(mix.table, h, ys[b, t], float(np.float32(mix.lam)), self_norm)
            q = mix.table.logq_all([a for a in h if a >= 0], V)
            bars[b, t] = row_bar(ys[b, t], q, back_of(mix.table, h), mix.lam, self_norm, ymix[b, t])
    return ymix, bars


def moved_share(ys, ymix, y):
    """the share of positions whose exact rank among all words differs between the plain and the mixed logits"""
    B, n, V = ys.shape
    S = np.arange(V)
    moved = sum(rc.exact_rank(ys[b, t], int(y[b, t]), S) != rc.exact_rank(ymix[b, t], int(y[b, t]), S) for b in range(B) for t in range(n))
    return moved / float(B * n)


def check_ranks(ranks, ymix, bars, y, index, tag, max_prefix=MAX_PREFIX):
    """every rank inside the oracle's interval over the mixed logits at delta = 2 DELTA + the position's bar; -1 exactly where the
    target has no such level.  -> (single-rank intervals, intervals)"""
    B, n = y.shape
    sets = {int(t): rc.level_sets(index, int(t), max_prefix) for t in np.unique(y)} if index is not None else None
    single = total = 0
    for b in range(B):
        for q in range(n):
            t = int(y[b, q])
            cols = sets[t] if sets is not None else [np.arange(ymix.shape[2])]
            for col, S in enumerate(cols):
                if S is None:
                    assert ranks[b, q, col] == -1, (tag, b, q, col)
                    continue
                lo, hi = rc.interval(ymix[b, q], t, S, 2 * rc.DELTA + bars[b, q])
                total += 1
                single += lo == hi
                assert lo <= ranks[b, q, col] <= hi, (tag, b, q, col, int(ranks[b, q, col]), lo, hi)
    return single, total


def check_lists(top_ids, top_logp, ymix, bars, y, ranks, self_norm, lam, tag):
    """the lists of a ranking call: ids equal the oracle's wherever its neighbouring mixed logits are more than 2 delta apart, log p
    within TOK_ATOL plus the bar (of the row-normalised mixture; self-normalised: y' + log1p(-lam)), most probable first, and
    column A < k exactly when the target is among the first k"""
    B, n, top = top_ids.shape
    for b in range(B):
        for q in range(n):
            ym = ymix[b, q]
            delta = 2 * rc.DELTA + bars[b, q]
            order = np.lexsort((np.arange(len(ym)), -ym))[:top + 1]
            v = ym[order]
            for i in range(top):
                clear = (i == 0 or v[i - 1] - v[i] > 2 * delta) and v[i] - v[i + 1] > 2 * delta
                if clear:
                    assert top_ids[b, q, i] == order[i], (tag, b, q, i)
            w = top_ids[b, q]
            want = ym[w] + np.log1p(-float(np.float32(lam))) if self_norm else ym[w] - (ym.max() + np.log(np.exp(ym - ym.max()).sum()))
            assert np.all(np.abs(top_logp[b, q] - want) <= TOK_ATOL + bars[b, q]), (tag, b, q)
            assert np.all(np.diff(top_logp[b, q]) <= 0)
            for k in (1, min(5, top)):
                assert (ranks[b, q, 0] < k) == (int(y[b, q]) in w[:k]), (tag, b, q, k)


def oracle_follow(lm, mix, prompt, bp_parent, bp_word, bp_nll, score, p, N, B, stop_id=None, first_set=None):
    """tests/test_gpu_complete.py oracle_follow under the mixture: the oracle teacher-forced on prompt p's device beams, every
    hypothesis's logits mixed with q(. | its last two words: the prompt's followed by its own); per frame the oracle's top-B from the
    device's parents -- frame 0 among ``first_set`` when given -- must be the device's kept set unless the gap at the cut is under
    TOL_E2E plus the bar, every kept word's nll within TOK_ATOL plus the bar of its row, and the final scores within their sum.
    bp_nll / score as the device reports them (self-normalised: -y').  -> (agreeing, ambiguous frames)"""
    sn = bool(lm.config["self_norm"])
    lam32 = float(np.float32(mix.lam))
    h, c = lm.zero_state(1)
    for w in prompt:
        h, c = lm.lstm_cell(np.array([w]), h, c)
    beam = [dict(h=h[0], c=c[0], s=0.0, fin=False, n=0, words=[int(w) for w in prompt], slack=0.0)]
    agree = amb = 0
    for k in range(N):
        Y = np.asarray(lm.project(np.stack([b["h"] for b in beam])), dtype=np.float64)
        cands, nlls, bars = [], [], []
        for j, b in enumerate(beam):
            if b["fin"]:
                cands.append((b["s"], j, -1))
                nlls.append(None)
                bars.append(0.0)
                continue
            hh = hist_of(b["words"])
            ym = mixed_logits(mix.table, hh, Y[j], lam32, sn)
            q = mix.table.logq_all([a for a in hh if a >= 0], len(ym))
            bars.append(row_bar(Y[j], q, back_of(mix.table, hh), mix.lam, sn, ym))
            nll = -ym if sn else (ym.max() + np.log(np.exp(ym - ym.max()).sum())) - ym
            nlls.append(nll)
            tot = b["s"] + nll
            if k == 0 and first_set is not None:
                allowed = np.asarray(first_set, dtype=np.int64)
                top = allowed[np.argsort(tot[allowed], kind="stable")[:B + 1]]
            else:
                top = np.argsort(tot, kind="stable")[:B + 1]
            cands.extend((float(tot[w]), j, int(w)) for w in top)
        cands.sort()
        q_rows = p * B + np.arange(B)
        dev = [(int(a), int(w)) for a, w in zip(bp_parent[k, q_rows], bp_word[k, q_rows])]
        if k == 0 and first_set is not None:
            dev = [d for d in dev if d[1] >= 0]                            # a set smaller than the beam pads with (-1, +inf)
        want_set = set((j, w) for _s, j, w in cands[:B])
        if set(dev) == want_set:
            agree += 1
        else:
            gap = cands[B][0] - cands[B - 1][0] if len(cands) > B else 0.0
            assert gap < TOL_E2E + max(bars), ("frame %d: kept set differs from the oracle's with a clear cut" % k, gap, set(dev) ^ want_set)
            amb += 1
        nb = []
        for i in range(B):
            j, w, n = int(bp_parent[k, q_rows[i]]), int(bp_word[k, q_rows[i]]), float(bp_nll[k, q_rows[i]])
            par = beam[j]
            if w < 0:
                if k == 0 and first_set is not None and not par["fin"]:
                    nb.append(dict(par, fin=True, s=np.inf))               # the padding of a small set: never expanded
                    continue
                assert par["fin"] and n == 0.0
                nb.append(dict(par))
                continue
            on = float(nlls[j][w])
            assert abs(n - on) <= TOK_ATOL + bars[j], (k, i, n, on)
            h2, c2 = lm.lstm_cell(np.array([w]), par["h"][None], par["c"][None])
            nb.append(dict(h=h2[0], c=c2[0], s=par["s"] + on, fin=stop_id is not None and w == stop_id, n=par["n"] + 1,
                           words=par["words"] + [w], slack=par["slack"] + bars[j]))
        beam = nb
    for i in range(B):
        if np.isfinite(beam[i]["s"]):
            assert abs(score[p * B + i] - beam[i]["s"]) <= TOK_ATOL * max(1, beam[i]["n"]) + beam[i]["slack"], (p, i)
    return agree, amb


def check_top(res, lm, mix, contexts, n, sets=None, tag=""):
    """predict_top / predict_reading's result against the oracle: after each context the mixed logits of its state with the history of
    its last two words; the words -- among ``sets[i]`` when given -- by mixed logit descending, lower id first: ids equal wherever the
    neighbouring logits are more than 2 delta apart, log p (row-normalised; self-normalised: y' + log1p(-lam)) within TOK_ATOL plus
    the bars.  -> the number of positions compared word for word"""
    sn = bool(lm.config["self_norm"])
    lam32 = float(np.float32(mix.lam))
    exact = 0
    for i, ctx in enumerate(contexts):
        h, c = lm.zero_state(1)
        for w in ctx:
            h, c = lm.lstm_cell(np.array([w]), h, c)
        y = np.asarray(lm.project(h), dtype=np.float64)[0]
        hh = hist_of(ctx)
        ym = mixed_logits(mix.table, hh, y, lam32, sn)
        bar = row_bar(y, mix.table.logq_all([a for a in hh if a >= 0], len(y)), back_of(mix.table, hh), mix.lam, sn, ym)
        delta = 2 * rc.DELTA + bar
        S = np.arange(len(y)) if sets is None or sets[i] is None else np.unique(np.asarray(sets[i], dtype=np.int64))
        order = S[np.lexsort((S, -ym[S]))]
        ids, logp = res[i]
        assert len(ids) == min(n, len(S)) and ids.dtype == np.int64 and logp.dtype == np.float64, (tag, i)
        v = ym[order]
        for k in range(len(ids)):
            if (k == 0 or v[k - 1] - v[k] > 2 * delta) and (k + 1 >= len(v) or v[k] - v[k + 1] > 2 * delta):
                assert ids[k] == order[k], (tag, i, k)
                exact += 1
        assert set(ids.tolist()) <= set(S.tolist())
        want = ym[ids] + np.log1p(-lam32) if sn else ym[ids] - (ym.max() + np.log(np.exp(ym - ym.max()).sum()))
        assert np.all(np.abs(logp - want) <= TOK_ATOL + bar), (tag, i, float(np.abs(logp - want).max()))
        assert np.all(np.diff(logp) <= 0)
    return exact


def handmade_table():
    """An order-3 table over 8 words with a context that has a back-off weight and no successors ((2, 3) and the word 6), successors
    without a weight ((4, 5) -> 0, 7; 5 -> 1), and a word without a unigram (7, reached only through the trigram (4, 5, 7))."""
    ent = {(0,): (-1.5, -0.25), (1,): (-2.0, 0.0), (2,): (-1.0, -0.5), (3,): (-2.5, -0.125), (4,): (-3.0, 0.0), (5,): (-1.25, 0.0),
           (6,): (-2.25, -0.75),
           (2, 3): (-0.5, -0.375), (3, 0): (-0.75, 0.0), (4, 5): (-0.25, 0.0), (5, 1): (-1.0, 0.0), (2, 2): (-1.75, -0.0625),
           (4, 5, 0): (-0.5, 0.0), (4, 5, 7): (-1.5, 0.0), (2, 2, 3): (-0.125, 0.0)}
    ks = sorted(ent, key=pack)
    return NGramTable([pack(k) for k in ks], [ent[k][0] for k in ks], [ent[k][1] for k in ks], 3)
