"""The yardstick of the left-context tests (tests/test_context_cpu.py, tests/test_gpu_context.py): the UNMODIFIED oracle decoding with a
history.

``oracle.jlm_oracle.static_decode`` / ``dynamic_decode`` call ``lm.zero_state(1)`` once and make their first ``lm.predict`` call with
the root's ``<eos>``.  :class:`PrimedLM` stands in for ``OracleDecoder.model`` for one call: its ``zero_state`` returns the oracle's
own state after ``hist[:-1]`` (hist = [<eos>] + context), its ``predict`` swaps the first call's index for ``hist[-1]``; ``project``
and ``config`` are the oracle's.  The n-best the oracle then returns is the expected decode with that left context:
:func:`chain_nll` -- the chain-rule sum of -log p over a path's words after the history, out-of-vocabulary lattice words as id 0 --
agrees with its 1-best score to 1e-9 (tests/test_context_cpu.py).
"""
import os
import tempfile

import numpy as np

from jlm_amd import config as jconfig, synth
from oracle import jlm_oracle as orc

EOS = 1
ALPHABET = 8
SCALE = 0.35
# name -> (V, H, E, mode, segments): the issue's two models, one D-softmax, one untied, and a tied model at H = 512 (the LSTM step's
# kernels are other code there) with a small vocabulary and embedding
MODELS = {
    "tied": (600, 64, 32, "tied", None),
    "vtable": (600, 64, 32, "vtable", [(32, 0, 200), (20, 200, None)]),
    "dsoftmax": (600, 64, 32, "dsoftmax", [(32, 0, 200), (20, 200, None)]),
    "untied": (600, 64, 32, "untied", None),
    "tied-h512": (300, 512, 16, "tied", None),
}
TIED = ("tied", "tied-h512")
BEAMS = (1, 5, 17)
_ROOTS = {}


def model_root(name):
    """the artefact directory of model ``name`` (written once per process)"""
    if name not in _ROOTS:
        V, H, E, mode, segs = MODELS[name]
        root = os.path.join(tempfile.gettempdir(), "jlm_test_ctx_%d" % os.getuid(), name)
        os.makedirs(root, exist_ok=True)
        cfg = synth.make_config(V, H, E, mode, segs)
        synth.write_lexicon(root, V, alphabet=ALPHABET)
        # (the gate pre-activations grow with sqrt(H): the scale keeps them where the H = 64 models have them, as tests/random_models.py)
        synth.write_experiment(root, 1, cfg, scale=SCALE * (64.0 / H) ** 0.5, seed=31)
        _ROOTS[name] = root
    return _ROOTS[name]


def oracle(name, dynamic=False):
    return (orc.OracleDynamicDecoder if dynamic else orc.OracleDecoder)(model_root(name), 1)


def sentences():
    """12 ragged inputs of 1 .. 10 kana"""
    return synth.make_ragged_sentences(12, 1, 10, seed=77, alphabet=ALPHABET)


def contexts(V, n=12, seed=5):
    """n mixed contexts of 0 .. 6 words: entry 0 empty, entry 1 with <eos> inside, entry 2 of 40 words, entry 3 None"""
    rng = np.random.RandomState(seed)
    out = [[int(x) for x in rng.randint(2, V, size=rng.randint(0, 7))] for _ in range(n)]
    out[0] = []
    out[1] = [int(rng.randint(2, V)), EOS, int(rng.randint(2, V))]
    out[2] = [int(x) for x in rng.randint(2, V, size=40)]
    out[3] = None
    return out


def ids_of(ctx):
    return [] if ctx is None else [int(w) for w in ctx]


def oracle_state(lm, words):
    """the oracle's (h, c) [1, H] after consuming ``words`` from the zero state"""
    h, c = lm.zero_state(1)
    for w in words:
        h, c = lm.lstm_cell([int(w)], h, c)
    return h, c


class PrimedLM:
    """``OracleDecoder.model`` for one decode with the history ``hist``"""

    def __init__(self, lm, hist):
        self.lm, self.hist = lm, [int(w) for w in hist]
        self.config = lm.config
        self.calls = 0

    def zero_state(self, rows=1):
        assert rows == 1
        return oracle_state(self.lm, self.hist[:-1])

    def predict(self, index, hidden, cell, vocab=None):
        if self.calls == 0:
            assert len(index) == 1
            index = [self.hist[-1]]
        self.calls += 1
        return self.lm.predict(index, hidden, cell, vocab)

    def project(self, hidden, vocab=None):
        return self.lm.project(hidden, vocab)


def primed_decode(o, text, ctx, **kw):
    """``o.decode(text, **kw)`` of an OracleDecoder with the left context ``ctx`` (word ids), the oracle's own code untouched"""
    if not len(text):
        return [(0.0, [])]
    lm = o.model
    o.lattice_vocab = None              # (the oracle keeps the reference's stale list across calls)
    o.model = PrimedLM(lm, [EOS] + ids_of(ctx))
    try:
        return o.decode(text, **kw)
    finally:
        o.model = lm
        o.lattice_vocab = None


def chain_nll(lm, hist, path):
    """the chain-rule -log p of the word ids ``path`` after the history ``hist`` (full vocabulary), per word, float64"""
    h, c = oracle_state(lm, hist[:-1])
    w, out = int(hist[-1]), []
    for t in path:
        pred, _y, h, c, _a, _b = lm.predict([w], h, c)
        out.append(-np.log(pred[0, int(t)]))
        w = int(t)
    return np.asarray(out, dtype=np.float64)


def path_ids(o, words):
    """lattice words -> the ids the model consumes (a word outside the vocabulary is id 0)"""
    return [o.w2i.get(w, 0) for w in words]


def check_nbest(got, want, tag):
    """the bars of tests/random_models.check: equal lengths, the same 1-best, every score within rtol 2e-6 / atol 2e-5"""
    assert len(got) == len(want), tag
    assert got[0][1] == want[0][1], (tag, got[0], want[0])
    np.testing.assert_allclose([x for x, _ in got], [x for x, _ in want], rtol=2e-6, atol=2e-5, err_msg=str(tag))


def set_root(name):
    jconfig.set_root(model_root(name))
