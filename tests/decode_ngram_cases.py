"""The yardstick of the decode-under-an-n-gram-mixture tests (tests/test_decode_ngram_cpu.py, tests/test_gpu_decode_ngram.py): the
UNMODIFIED oracle behind a proxy, built on tests/context_cases.PrimedLM.

The oracle's ``predict(index, hidden, cell)`` sees a row's last word and its previous state, but not its path.  :class:`NGramLM`
therefore keeps a dict from ``h_new[row].tobytes()`` to the last words of the row's history, and looks the parent's up under
``hidden[row].tobytes()``; the root is the zero or primed state, with the history [<eos>] + ctx.  Two rows with identical float64
states have identical histories (asserted where a state is met twice).  Every ``predict`` returns
``(1 - lam) pred + lam exp(q(. | hist))`` over all V words from ``NGramTable.logq_all``.

The tables (:func:`mix`) are estimated from a small "corpus" made of the word sequences on the plain oracle's lower-ranked paths
(beam 17) of the 12 ragged inputs, repeated REPS times: the n-gram model favours conversions the LSTM ranks low.
"""
import numpy as np

from jlm_amd.ngram import NGramMix, estimate
from tests import context_cases as cc
from tests import decode_cache_cases as dc
from tests.context_cases import MODELS, sentences                        # noqa: F401  (the models and the 12 ragged inputs)

EOS = cc.EOS
LAM = 0.5
REPS = 3
ORDERS = (2, 3)
contexts = dc.contexts                  # words the lattice offers: entry 0 [], entry 3 None, entry 1 holds <eos>, entry 2 of 40 words

_MIX = {}


def corpus(name):
    """the id stream: every lower-ranked path of every input, each ending in <eos>, REPS times over"""
    o = cc.oracle(name)
    ids = []
    for text in sentences():
        for _s, path in o.decode(text, topN=17, beam_width=17)[1:]:
            ids += cc.path_ids(o, path) + [EOS]
    return np.asarray(ids * REPS, dtype=np.int64)


def mix(name, order, lam=LAM):
    """the NGramMix of model ``name`` at ``order`` (estimated once per process)"""
    if (name, order, lam) not in _MIX:
        _MIX[(name, order, lam)] = NGramMix(estimate(corpus(name), MODELS[name][0], order), lam)
    return _MIX[(name, order, lam)]


class NGramLM(cc.PrimedLM):
    """``OracleDecoder.model`` for one decode with the history ``hist`` under the n-gram mixture ``mix``"""

    def __init__(self, lm, hist, mix):
        super().__init__(lm, hist)
        self.table, self.lam = mix.table, float(mix.lam)
        self.tail_of = {}               # state bytes -> the last two words of the history that led to it
        self._q = {}

    def _see(self, h_row, tail):
        key = np.ascontiguousarray(h_row, dtype=np.float64).tobytes()
        assert self.tail_of.setdefault(key, tail) == tail, "two histories behind one state"

    def zero_state(self, rows=1):
        h, c = super().zero_state(rows)
        self._see(h[0], tuple(self.hist[:-1][-2:]))
        return h, c

    def q(self, tail, V):
        if tail not in self._q:
            self._q[tail] = np.exp(self.table.logq_all(tail, V))
        return self._q[tail]

    def predict(self, index, hidden, cell, vocab=None):
        assert vocab is None
        words = [self.hist[-1]] if self.calls == 0 else [int(w) for w in index]
        pred, y, h, c, a, b = super().predict(index, hidden, cell, vocab)
        pred = np.array(pred, dtype=np.float64)
        for r, w in enumerate(words):
            parent = self.tail_of[np.ascontiguousarray(hidden[r], dtype=np.float64).tobytes()]
            tail = (parent + (w,))[-2:]
            self._see(h[r], tail)
            pred[r] = (1.0 - self.lam) * pred[r] + self.lam * self.q(tail, pred.shape[1])
        return pred, y, h, c, a, b


def mixed_decode(o, text, ctx, mix, **kw):
    """``o.decode(text, **kw)`` of an OracleDecoder with the left context ``ctx`` under the mixture, the oracle's own code untouched"""
    if not len(text):
        return [(0.0, [])]
    lm = o.model
    o.lattice_vocab = None
    o.model = NGramLM(lm, [EOS] + cc.ids_of(ctx), mix)
    try:
        return o.decode(text, **kw)
    finally:
        o.model = lm
        o.lattice_vocab = None


def chain_nll_mix(lm, hist, path, mix):
    """the chain-rule -log p_mix of the word ids ``path`` after ``hist``, per word, float64 (NGramTable.logq, word by word)"""
    plain = cc.chain_nll(lm, hist, path)
    seq = [int(w) for w in hist] + [int(w) for w in path]
    out = []
    for t, w in enumerate(path):
        q = mix.table.logq(seq[:len(hist) + t], int(w))
        out.append(-np.log((1.0 - mix.lam) * np.exp(-plain[t]) + mix.lam * np.exp(q)))
    return np.asarray(out, dtype=np.float64)
