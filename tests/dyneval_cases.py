"""Shared by tests/test_dyneval_cpu.py, tests/test_gpu_dyneval_kernels.py and tests/test_gpu_dyneval.py: the toy model dynamic
evaluation is tried on (tied, V = 600, H = 64, E = 32, three epochs of the float64 trainer on the Markov walk of tests/train_cases.py),
an in-domain stream and a shifted one, and the three-line restatement of the two update rules."""
import numpy as np

from jlm_amd import config as jconfig, train as T
from tests import train_cases as tc

V = tc.MARKOV_V
N_EVAL = 3001                       # 3 000 scored tokens at B = 1, T = 5
_cache = {}


def table(seed=3):
    """the walk's transition table, as tc.markov_stream draws it"""
    return np.random.RandomState(seed).randint(1, V, (V, 4))


def shifted_table(nxt):
    """half of the states' transition rows re-drawn: rows = RandomState(5).rand(V) < 0.5, then those rows from the same generator"""
    rng = np.random.RandomState(5)
    rows = rng.rand(V) < 0.5
    out = nxt.copy()
    out[rows] = rng.randint(1, V, (int(rows.sum()), 4))
    return out


def walk(nxt, n, seed):
    rng = np.random.RandomState(seed)
    ks = rng.choice(4, size=n, p=tc.MARKOV_P)
    out, cur = np.empty(n, dtype=np.int64), 1
    for i in range(n):
        cur = nxt[cur, ks[i]]
        out[i] = cur
    return out


def streams():
    """-> (in-domain, shifted): N_EVAL ids each, the same choices k_i on the trained table and on the shifted one"""
    if "streams" not in _cache:
        nxt = table()
        _cache["streams"] = (walk(nxt, N_EVAL, 11), walk(shifted_table(nxt), N_EVAL, 11))
    return _cache["streams"]


def trial_model():
    """-> (cfg, weights): B = 32, T = 10, lr 5e-3, no dropout, three epochs over tc.markov_stream(48032); trained once per process"""
    if "model" not in _cache:
        cfg = tc.small_cfg("tied", V, 64, 32, False)
        st = T.ReferenceStepper(cfg, T.init_weights(cfg, None, 101), 32, 10, lr=5e-3, dropout=1.0, norm_weight=0.0)
        train = tc.markov_stream(48032, 3)
        for _ in range(3):
            T.run_epoch(st, train, 32, 10, True, 0)
        _cache["model"] = (cfg, st.weights())
    return _cache["model"]


def write_experiment(root, cfg, weights, experiment_id=1):
    """the model as an experiment under ``root`` (config.json and the weight dump) -> its id; jlm_amd.config points at ``root``"""
    jconfig.set_root(root)
    T.write_experiment(experiment_id, cfg, weights)
    return experiment_id


def restated(rule, w, g, w0, rms, mean, lr, lam, eps):
    """both rules in three lines of numpy (float64 arrays)"""
    if rule == "sgd":
        return w - lr * g + lam * (w0 - w)
    coefficient = np.minimum(lam * rms / mean, 1.0)
    return w - lr * g / (rms + eps) + coefficient * (w0 - w)


def flat_mean(stats):
    """mean over every element of a dump-shaped dict, the test's own way"""
    return float(np.concatenate([a.astype(np.float64).reshape(-1) for _k, a in tc.flat_items(stats)]).mean())
