"""The yardstick of the decode-under-a-memory tests (tests/test_decode_memory_cpu.py, tests/test_gpu_decode_memory.py): the UNMODIFIED
oracle behind a proxy, built on tests/context_cases.PrimedLM in the manner of tests/decode_cache_cases.CachedLM.

The memory of model ``name`` (:func:`store`) is one pass of the oracle's own ``lstm_cell`` over the id stream of
tests/decode_ngram_cases.corpus(name) taken once (REPS = 1; 717 .. 813 entries): entry i is (the state after consuming the stream's
word i - 1 from the zero state, <eos> in front; word i).  :class:`MemoryLM`'s every ``predict`` returns
``(1 - lam) pred + lam c_r`` with ``c_r`` the float64 definition of DESIGN.md section 30 over T_K(r) by the definition's total order,
and records, per query row, whether the K-th and the (K + 1)-th score are further apart than twice the row's end-to-end score bar
(tests/decode_memory_budget.py): an input all of whose rows are is *separable* -- a device whose scores are within their bars picks
the very neighbour sets of the oracle.  :func:`chain_interval` is the float64 interval of a path's chain score when every entry within
twice the bar of the K-th is taken in or out of T_K, whichever lowers or raises the word's mass (section 29's rank intervals).
"""
import numpy as np

from tests import context_cases as cc
from tests import decode_cache_cases as dc
from tests import decode_ngram_cases as ng
from tests.context_cases import MODELS, sentences                        # noqa: F401  (the models and the 12 ragged inputs)
from tests.decode_memory_budget import score_bars

EOS = cc.EOS
THETA, LAM = 0.6, 0.5
K_ALL, K_SMALL = 1024, 16               # K >= N: the whole memory votes; K = 16: a retrieval proper
contexts = dc.contexts                  # words the lattice offers: entry 0 [], entry 3 None, entry 1 holds <eos>, entry 2 of 40 words

_STORE = {}


def store(name):
    """(ids [N] int64 -- the stream --, keys [N, H] float64, words [N] int64) of model ``name`` (built once per process)"""
    if name not in _STORE:
        ids = ng.corpus(name)
        ids = ids[:len(ids) // ng.REPS]
        lm = cc.oracle(name).model
        h, c = lm.zero_state(1)
        keys, w = [], EOS
        for t in ids:
            h, c = lm.lstm_cell([int(w)], h, c)
            keys.append(np.array(h[0], dtype=np.float64))
            w = int(t)
        _STORE[name] = (ids, np.asarray(keys), np.asarray(ids, dtype=np.int64))
    return _STORE[name]


def streams(name):
    """the store's stream as Memory.build takes it: (inputs [1, N], targets [1, N])"""
    ids = store(name)[0]
    return np.concatenate([[EOS], ids[:-1]])[None, :], ids[None, :]


def neighbours(h, keys, theta, K):
    """T_K by the definition's total order -> (order [N] best first, s [N] float64, n_q)"""
    s = float(theta) * (keys @ np.asarray(h, dtype=np.float64)) + 0.0
    return np.lexsort((np.arange(len(s)), -s)), s, min(int(K), len(s))


class MemoryLM(cc.PrimedLM):
    """``OracleDecoder.model`` for one decode with the history ``hist`` under the memory (keys, words)"""

    def __init__(self, lm, hist, keys, words, K, theta=THETA, lam=LAM):
        super().__init__(lm, hist)
        self.keys, self.words, self.K, self.theta, self.lam = keys, words, int(K), float(theta), float(lam)
        self.margins = []               # per query row with K < N: (K-th score - (K + 1)-th score) - 2 bar

    def predict(self, index, hidden, cell, vocab=None):
        assert vocab is None
        pred, y, h, c, a, b = super().predict(index, hidden, cell, vocab)
        pred = np.array(pred, dtype=np.float64)
        for q in range(h.shape[0]):
            order, s, n = neighbours(h[q], self.keys, self.theta, self.K)
            top = order[:n]
            if n < len(order):
                self.margins.append(s[order[n - 1]] - s[order[n]] - 2.0 * score_bars(h[q], self.keys, self.theta).max())
            e = np.exp(s[top] - s[top[0]])
            cq = np.zeros(pred.shape[1])
            np.add.at(cq, self.words[top], e / e.sum())
            pred[q] = (1.0 - self.lam) * pred[q] + self.lam * cq
        return pred, y, h, c, a, b


def memory_decode(o, text, ctx, name, K, theta=THETA, lam=LAM, **kw):
    """``o.decode(text, **kw)`` of an OracleDecoder with the left context ``ctx`` under the memory of ``name``, the oracle's own code
    untouched -> (n-best, separable)"""
    if not len(text):
        return [(0.0, [])], True
    _ids, keys, words = store(name)
    lm = o.model
    o.lattice_vocab = None
    o.model = proxy = MemoryLM(lm, [EOS] + cc.ids_of(ctx), keys, words, K, theta, lam)
    try:
        return o.decode(text, **kw), all(m > 0.0 for m in proxy.margins)
    finally:
        o.model = lm
        o.lattice_vocab = None


def chain_interval(lm, hist, path, keys, words, K, theta=THETA, lam=LAM):
    """(lo, nominal, hi): the chain-rule sum of -log p_mix of the word ids ``path`` after ``hist`` by the definition, and the interval
    it moves in when, per step, every entry whose float64 score is within twice the row's bar of the boundary between the K-th and
    the (K + 1)-th is taken in or out of T_K, whichever raises or lowers the word's mass"""
    h, c = cc.oracle_state(lm, hist[:-1])
    w, lo, mid, hi = int(hist[-1]), 0.0, 0.0, 0.0
    for t in path:
        pred, _y, h, c, _a, _b = lm.predict([w], h, c)
        p_lm, t = float(pred[0, int(t)]), int(t)
        order, s, n = neighbours(h[0], keys, theta, K)
        e = np.exp(s - s[order[0]])
        rank = np.empty(len(s), dtype=np.int64)
        rank[order] = np.arange(len(s))
        inside, same = rank < n, words == t
        amb = np.zeros(len(s), dtype=bool)
        if n < len(s):
            thr = 2.0 * score_bars(h[0], keys, theta).max()
            amb = np.where(inside, s - s[order[n]] <= thr, s[order[n - 1]] - s <= thr)
        sure = inside & ~amb
        m_sure, z_sure = e[sure & same].sum(), e[sure].sum()
        m_amb, z_other = e[amb & same].sum(), e[amb & ~same].sum()
        c_mid = e[inside & same].sum() / e[inside].sum()
        c_hi = (m_sure + m_amb) / (z_sure + m_amb) if z_sure + m_amb > 0.0 else 0.0
        c_lo = m_sure / (z_sure + z_other) if z_sure + z_other > 0.0 else 1.0
        assert c_lo <= c_mid * (1 + 1e-12) and c_mid <= c_hi * (1 + 1e-12), (c_lo, c_mid, c_hi)
        lo -= np.log((1.0 - lam) * p_lm + lam * c_hi)
        mid -= np.log((1.0 - lam) * p_lm + lam * c_mid)
        hi -= np.log((1.0 - lam) * p_lm + lam * c_lo)
        w = t
    return lo, mid, hi
