"""The yardstick of the unfinished-reading tests (tests/test_predict_convert_cpu.py, tests/test_gpu_predict_convert.py): the UNMODIFIED
oracle, listened to.

``oracle.jlm_oracle.static_decode`` makes one ``lm.predict`` call per frame, in frame order, and ``OracleDecoder.last_trace`` keeps each
frame's scores and back-pointers.  :class:`RecordingLM` stands in for ``OracleDecoder.model`` for one call (around
``context_cases.PrimedLM``, which gives the decode its history) and keeps the ``pred`` of every call: frame s's rows are the
full-vocabulary distributions after the hypotheses the beam kept there.  :func:`oracle_predict` then enumerates the candidates exactly
as DESIGN.md section 16 defines them -- tail start s ascending, extension word in ReadingIndex order, slot ascending -- and sorts them
stably by score.
"""
import math

import numpy as np

from jlm_amd.data import Vocab
from jlm_amd.readings import ReadingIndex
from tests import context_cases as cc

TOPN = 10
SEPARATION = 1e-4          # a position is compared word for word when its yardstick score is further than this from both neighbours
MAX_EXEMPT = 2             # positions per (model, beam) that may be closer (measured: one pair 5.3e-5 apart, tied-h512 at beam 1)
_INDEX = {}


def index_of(name):
    """the ReadingIndex of model ``name``'s vocabulary (one per process)"""
    if name not in _INDEX:
        cc.set_root(name)                                   # (Vocab reads the lexicon under the configured root)
        _INDEX[name] = ReadingIndex(Vocab(cc.MODELS[name][0]))
    return _INDEX[name]


def inputs():
    """context_cases' 12 ragged inputs and one empty input"""
    return cc.sentences() + [""]


def contexts(V, seed=5):
    """one context per input of :func:`inputs`"""
    return cc.contexts(V, n=13, seed=seed)


class RecordingLM:
    """``OracleDecoder.model`` for one decode: forwards everything, keeps the ``pred`` of every ``predict`` call"""

    def __init__(self, lm):
        self.lm = lm
        self.config = lm.config
        self.preds = []

    def zero_state(self, rows=1):
        return self.lm.zero_state(rows)

    def predict(self, index, hidden, cell, vocab=None):
        out = self.lm.predict(index, hidden, cell, vocab)
        self.preds.append(out[0])
        return out

    def project(self, hidden, vocab=None):
        return self.lm.project(hidden, vocab)


def _path(ends, trace, f, k):
    out = []
    while f >= 0:
        _scores, prevs, nodes = trace[f]
        out.append(ends[f][nodes[k]][3])
        f, k = prevs[k]
    out.reverse()
    return [w for w in out if w != "<eos>"]


def oracle_predict(o, index, text, ctx=None, beam=10, topN=TOPN):
    """-> (conversions, candidates): the oracle's n-best of ``text`` after the context ``ctx`` (word ids), and EVERY candidate
    (score, [word, ...]) of its unfinished last word, stably sorted by score in candidate order (callers cut it at topN and may look at
    the entry behind)"""
    lm = o.model
    hist = [cc.EOS] + cc.ids_of(ctx)
    if not len(text):
        h, c = cc.oracle_state(lm, hist[:-1])
        pred = lm.predict([hist[-1]], h, c)[0]
        _lo, mid, hi = index.ranges("")
        cands = [(-math.log(pred[0, int(w)]), [o.i2w[int(w)]]) for w in index.ids[mid:hi]]
        cands.sort(key=lambda x: x[0])
        return [(0.0, [])], cands
    rec = RecordingLM(cc.PrimedLM(lm, hist))
    o.lattice_vocab = None
    o.model = rec
    try:
        conv = o.decode(text, topN=topN, beam_width=beam)
    finally:
        o.model = lm
        o.lattice_vocab = None
    trace, ends = o.last_trace, o.backward_lookup
    assert len(rec.preds) == len(text) + 1 == len(trace)
    cands = []
    for s in range(len(text)):
        _lo, mid, hi = index.ranges(text[s:])
        scores = trace[s][0]
        assert rec.preds[s].shape[0] == len(scores)
        for w in index.ids[mid:hi]:
            for k in range(len(scores)):
                cands.append((scores[k] - math.log(rec.preds[s][k, int(w)]), s, k, int(w)))
    cands.sort(key=lambda x: x[0])                         # stable: ties keep (s, word order, slot)
    return conv, [(sc, _path(ends, trace, s, k) + [o.i2w[w]]) for sc, s, k, w in cands]


def separated(cands, topN=TOPN):
    """per position < min(topN, len): is its score further than SEPARATION from both neighbours (the entry behind the list included)"""
    sc = [c[0] for c in cands[:topN + 1]]
    out = []
    for i in range(min(topN, len(cands))):
        left = i == 0 or sc[i] - sc[i - 1] > SEPARATION
        right = i + 1 >= len(sc) or sc[i + 1] - sc[i] > SEPARATION
        out.append(left and right)
    return out


def check_predictions(got, cands, tag, topN=TOPN):
    """the end-to-end bar: the same length, sorted scores within the suite's bar (rtol 2e-6 / atol 2e-5), the same words at every
    separated position.  -> the number of positions that were not separated"""
    want = cands[:topN]
    assert len(got) == len(want), (tag, len(got), len(want))
    gs = [x for x, _ in got]
    assert gs == sorted(gs), tag
    np.testing.assert_allclose(gs, [x for x, _ in want], rtol=2e-6, atol=2e-5, err_msg=str(tag))
    sep = separated(cands, topN)
    for i, ok in enumerate(sep):
        if ok:
            assert got[i][1] == want[i][1], (tag, i, got[i], want[i])
    return sep.count(False)


_YARD = {}


def yardstick(name, beam, with_ctx, seed=5):
    """[(conversions, the first TOPN + 1 candidates)] over :func:`inputs` for one (model, beam), computed once per process"""
    key = (name, beam, bool(with_ctx), seed)
    if key not in _YARD:
        o, index = cc.oracle(name), index_of(name)
        ctxs = contexts(cc.MODELS[name][0], seed) if with_ctx else [None] * 13
        out = []
        for text, ctx in zip(inputs(), ctxs):
            conv, cands = oracle_predict(o, index, text, ctx, beam)
            out.append((conv, cands[:TOPN + 1]))
        _YARD[key] = out
    return _YARD[key]
