"""The yardstick of the ranking tests (tests/test_rank_cpu.py, tests/test_gpu_rank.py): the definition of include/jlm_hip.h
jlm_rank_rows stated directly in numpy over the oracle's float64 logits, on the models of tests/context_cases.py.

A device logit differs from the oracle's by rounding, so a device rank is compared with the INTERVAL of ranks the oracle's logits
leave open at DELTA = 1e-4, the project's stated bar for step logits against the reference: within a level S of target t

    lo = #{ w in S : y[w] > y[t] + DELTA },    hi = #{ w in S : y[w] >= y[t] - DELTA } - 1      (t itself is in S)

Every word the device may have moved across the target lies between the two.  tests/test_rank_cpu.py asserts the condition that keeps
this from being vacuous: the interval is a single rank for at least 80 % of the (token, level) entries of each model.
"""
import numpy as np

from tests import context_cases as cc
from tests import predict_cases as pc

DELTA = 1e-4
MAX_PREFIX = 8
MODELS = ("tied", "vtable", "dsoftmax", "untied")
GPU_MODELS = MODELS + ("tied-h512",)
_LOGITS, _BOUNDS = {}, {}


def sequences(V, seed=19):
    """five rows of 1 .. 12 words, an empty one and a 40-word row; <unk> and <eos> (no reading) occur as targets"""
    rng = np.random.RandomState(seed)
    out = [[int(x) for x in rng.randint(2, V, size=n)] for n in (3, 12, 1, 0, 7, 5, 40)]
    out[1][4], out[1][9], out[4][6], out[6][17] = cc.EOS, 0, cc.EOS, 0
    return out


def oracle_logits(name):
    """per sequence the oracle's logits [len, V] float64 of every step: step 0 consumes <eos> from the zero state (computed once)"""
    if name not in _LOGITS:
        lm = cc.oracle(name).model
        out = []
        for s in sequences(cc.MODELS[name][0]):
            h, c = lm.zero_state(1)
            w, ys = cc.EOS, []
            for t in s:
                _pred, y, h, c, _a, _b = lm.predict([w], h, c)
                ys.append(np.asarray(y, dtype=np.float64).reshape(-1))
                w = int(t)
            out.append(np.stack(ys) if ys else np.zeros((0, cc.MODELS[name][0])))
        _LOGITS[name] = out
    return _LOGITS[name]


def level_sets(index, t, max_prefix):
    """the word sets of target t's columns by a brute-force scan of the readings: [A, prefix 0 .. max_prefix, X], None where the
    target has no such level"""
    V = index.V
    sets = [np.arange(V)] + [None] * (max_prefix + 2)
    where = np.flatnonzero(index.ids == t)
    if len(where):
        r = index.readings[int(where[0])]
        for j in range(min(len(r), max_prefix) + 1):
            sets[1 + j] = np.array([int(i) for q, i in zip(index.readings, index.ids) if q.startswith(r[:j])], dtype=np.int64)
        sets[-1] = np.array([int(i) for q, i in zip(index.readings, index.ids) if q == r], dtype=np.int64)
    return sets


def exact_rank(y, t, S):
    """the definition on one row"""
    S = np.asarray(S, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        return int(np.count_nonzero(y[S] > y[t]) + np.count_nonzero((y[S] == y[t]) & (S < t)))


def interval(y, t, S, delta=DELTA):
    S = np.asarray(S, dtype=np.int64)
    return int(np.count_nonzero(y[S] > y[t] + delta)), int(np.count_nonzero(y[S] >= y[t] - delta)) - 1


def bounds(name, max_prefix=MAX_PREFIX):
    """per sequence (lo, hi) int64 [len, max_prefix + 3] of the oracle's intervals, -1 / -1 where the target has no such level"""
    key = (name, max_prefix)
    if key not in _BOUNDS:
        index = pc.index_of(name)
        sets = {}
        out = []
        for s, ys in zip(sequences(cc.MODELS[name][0]), oracle_logits(name)):
            lo = np.full((len(s), max_prefix + 3), -1, dtype=np.int64)
            hi = lo.copy()
            for i, t in enumerate(s):
                if t not in sets:
                    sets[t] = level_sets(index, t, max_prefix)
                for col, S in enumerate(sets[t]):
                    if S is not None:
                        lo[i, col], hi[i, col] = interval(ys[i], t, S)
            out.append((lo, hi))
        _BOUNDS[key] = out
    return _BOUNDS[key]


def check_in_bounds(got, name, max_prefix=MAX_PREFIX, columns=None):
    """every rank of ``got`` (LSTM_Model.rank's result for sequences()) inside the oracle's interval, -1 exactly where a level is absent"""
    for k, (g, (lo, hi)) in enumerate(zip(got, bounds(name, max_prefix))):
        if columns is not None:
            lo, hi = lo[:, columns], hi[:, columns]
        assert g.shape == lo.shape and g.dtype == np.int32, (name, k, g.shape, lo.shape)
        bad = np.argwhere((g < lo) | (g > hi))
        assert not len(bad), (name, k, bad[:5].tolist(), g[tuple(bad[0])], lo[tuple(bad[0])], hi[tuple(bad[0])])


def reading_len(index, t):
    where = np.flatnonzero(index.ids == t)
    return len(index.readings[int(where[0])]) if len(where) else 0

