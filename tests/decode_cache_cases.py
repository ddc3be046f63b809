"""The yardstick of the decode-under-the-cache tests (tests/test_decode_cache_cpu.py, tests/test_gpu_decode_cache.py): the UNMODIFIED
oracle behind a proxy, built like tests/context_cases.PrimedLM.

:class:`CachedLM` primes ``zero_state`` and the first ``predict`` as PrimedLM does, and every ``predict`` returns
``(1 - lam) pred + lam c(h_new)`` with c from the float64 definition over the oracle's OWN window states:
the last N pairs (h_j, hist[j + 1]) of hist = [<eos>] + ctx, h_j the oracle's state after hist[j].  An empty window returns pred.

The contexts (:func:`contexts`) are made of words the input's lattice offers -- the words of the plain oracle's lower-ranked paths --
because random ids over V = 600 almost never meet an edge and the test would show nothing.
"""
import atexit
import os
import shutil
import tempfile

import numpy as np

from jlm_amd import config as jconfig, synth
from oracle import jlm_oracle as orc
from tests import context_cases as cc
from tests.context_cases import MODELS, oracle_state, sentences          # noqa: F401  (the models and the 12 ragged inputs)

EOS = cc.EOS
THETA, LAM = 0.6, 0.5                   # one theta, one lambda: chosen so that the ORACLE's 1-best moves (test_decode_cache_cpu.py)
SIZES = (16, 64)                        # N: 16 truncates the 40-word context, 64 does not


_ROOTS = {}


def model_root(name):
    """context_cases.model_root's artefacts (the same seeds: the same weights) in a directory of THIS process: that module writes a
    shared directory at every process's first use, which a parallel test worker may be reading meanwhile"""
    if name not in _ROOTS:
        if not _ROOTS:
            _ROOTS[None] = tempfile.mkdtemp(prefix="jlm_test_dcache_")
            atexit.register(shutil.rmtree, _ROOTS[None], ignore_errors=True)
        V, H, E, mode, segs = MODELS[name]
        root = os.path.join(_ROOTS[None], name)
        os.makedirs(root, exist_ok=True)
        synth.write_lexicon(root, V, alphabet=cc.ALPHABET)
        synth.write_experiment(root, 1, synth.make_config(V, H, E, mode, segs), scale=cc.SCALE * (64.0 / H) ** 0.5, seed=31)
        _ROOTS[name] = root
    return _ROOTS[name]


def oracle(name):
    return orc.OracleDecoder(model_root(name), 1)


def set_root(name):
    jconfig.set_root(model_root(name))


def window(lm, ctx, N):
    """(h [n, H] float64, words [n]) of the window of hist = [<eos>] + ctx: the last min(len(ctx), N) pairs, oldest first"""
    hist = [EOS] + [int(w) for w in ctx]
    hs = []
    h, c = lm.zero_state(1)
    for w in hist[:-1]:
        h, c = lm.lstm_cell([int(w)], h, c)
        hs.append(h[0].copy())
    n = min(len(ctx), N)
    H = lm.hidden_size
    return (np.asarray(hs[len(hs) - n:], dtype=np.float64).reshape(n, H), np.asarray(hist[1:][len(ctx) - n:], dtype=np.int64))


def cache_probs(keys, words, h, theta, V):
    """c [rows, V]: the float64 definition for the query states h [rows, H]"""
    s = theta * (np.asarray(h, dtype=np.float64) @ keys.T)
    e = np.exp(s - s.max(axis=1, keepdims=True))
    c = np.zeros((h.shape[0], V))
    for q in range(h.shape[0]):
        np.add.at(c[q], words, e[q] / e[q].sum())
    return c


class CachedLM(cc.PrimedLM):
    """``OracleDecoder.model`` for one decode with the history ``hist`` under the continuous cache"""

    def __init__(self, lm, hist, N, theta=THETA, lam=LAM):
        super().__init__(lm, hist)
        self.theta, self.lam = float(theta), float(lam)
        self.keys, self.words = window(lm, self.hist[1:], N)

    def predict(self, index, hidden, cell, vocab=None):
        assert vocab is None
        pred, y, h, c, a, b = super().predict(index, hidden, cell, vocab)
        if len(self.words) and self.lam > 0.0:
            pred = (1.0 - self.lam) * pred + self.lam * cache_probs(self.keys, self.words, h, self.theta, pred.shape[1])
        return pred, y, h, c, a, b


def cached_decode(o, text, ctx, N, theta=THETA, lam=LAM, **kw):
    """``o.decode(text, **kw)`` of an OracleDecoder with the left context ``ctx`` under the cache, the oracle's own code untouched"""
    if not len(text):
        return [(0.0, [])]
    lm = o.model
    o.lattice_vocab = None
    o.model = CachedLM(lm, [EOS] + cc.ids_of(ctx), N, theta, lam)
    try:
        return o.decode(text, **kw)
    finally:
        o.model = lm
        o.lattice_vocab = None


def chain_nll_mix(lm, hist, path, N, theta=THETA, lam=LAM):
    """the chain-rule -log p_mix of the word ids ``path`` after ``hist``, per word, float64"""
    proxy = CachedLM(lm, hist, N, theta, lam)
    h, c = proxy.zero_state(1)
    w, out = int(hist[-1]), []
    proxy.calls = 1                         # (the first word is given here, not swapped in)
    for t in path:
        pred, _y, h, c, _a, _b = proxy.predict([w], h, c)
        out.append(-np.log(pred[0, int(t)]))
        w = int(t)
    return np.asarray(out, dtype=np.float64)


_CTX = {}


def contexts(name):
    """12 contexts for the 12 inputs of model ``name``: the ids of the words on the plain oracle's lower-ranked paths of that input
    (beam 17), in path order -- words the lattice offers again.  Entry 0 is [], entry 3 None, entry 1 holds <eos>, entry 2 is cycled
    to 40 words (longer than N = 16)."""
    if name not in _CTX:
        o = oracle(name)
        out = []
        for i, text in enumerate(sentences()):
            words = [w for _s, path in o.decode(text, topN=17, beam_width=17)[1:] for w in path]
            ids = [o.w2i.get(w, 0) for w in words][:8] or [2 + i]
            out.append(ids)
        out[0], out[3] = [], None
        out[1] = out[1][:2] + [EOS] + out[1][2:]
        out[2] = [out[2][k % len(out[2])] for k in range(40)]
        _CTX[name] = out
    return _CTX[name]
