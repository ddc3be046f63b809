"""Helpers the truncated-sampling tests share (tests/test_generate_truncated_cpu.py, tests/test_gpu_generate_truncated.py): the kernel
test's inputs, the float64 judgement of one truncated draw, and the oracle teacher-forced on a set of draws."""
import numpy as np

from jlm_amd import generate as G
from tests.gpu_rows import lse

# the kernel-level cases (tests/test_gpu_generate_truncated.py); the CPU suite checks their cuts are unambiguous
N_COLS = [1, 63, 64, 65, 1025, 100003]
TEMPERATURES = [0.05, 1.0, 10.0]
KP = [(1, None), (2, None), (40, None), (None, 0.9), (None, 0.5), (None, 1e-6), (50, 0.9), ("V", 1.0)]
TOL_KERNEL = 1e-9


def kernel_logits(n_cols):
    """the kernel test's rows for one n_cols: 3 N(0, 1) as f32 from RandomState(n_cols)"""
    R = 96 if n_cols <= 1025 else 24
    return (np.random.RandomState(n_cols).standard_normal((R, n_cols)) * 3).astype(np.float32)


def rank_order(y):
    """word ids by (y descending, id ascending)"""
    return np.lexsort((np.arange(len(y)), -np.asarray(y, dtype=np.float64)))


def masses(y, temperature, f32=True):
    """float64 masses; f32: the tempered argument formed in float32 from f32 logits as the kernel forms it"""
    if f32:
        y = np.asarray(y, dtype=np.float32)
        return np.exp(((y - y.max()) * np.float32(1.0 / temperature)).astype(np.float64))
    y = np.asarray(y, dtype=np.float64)
    return np.exp((y - y.max()) / temperature)


def cut_distance(mass_ranked, top_p):
    """how close p S_K comes to a boundary of the rank-order cumulative mass of K, relative to S_K"""
    c = np.cumsum(mass_ranked)
    return float(np.abs(c - top_p * c[-1]).min() / c[-1])


def _draw_fits(mass, keep, u, got, tol):
    """'exact' when `got` is the inverse-CDF draw over the kept masses, 'near' when u S_kept lies within tol S_kept of got's interval"""
    if not keep[got]:
        return None
    m = np.where(keep, mass, 0.0)
    if G.inverse_cdf(m, u) == got:
        return "exact"
    c = np.cumsum(m)
    S, t = c[-1], u * c[-1]
    lo = c[got - 1] if got > 0 else 0.0
    if m[got] > 0 and lo - tol * S <= t <= c[got] + tol * S:
        return "near"
    return None


def judge_draw(y, temperature, top_k, top_p, u, got, tol, y_tol=0.0, f32=True, order=None, mass=None):
    """One draw `got` against the float64 rule (jlm_amd/generate.py) over logits y: -> True when it is the rule's draw, False when it
    differs but is excused -- u S_kept within a relative `tol` of a boundary of the kept CDF, p S_K within a relative `tol` of a
    boundary of the rank-order cumulative mass (the draw must then fit a cut one word shorter or longer), or, with y_tol, the logits
    at ranks k and k + 1 closer than y_tol.  AssertionError for anything else."""
    V = len(y)
    assert 0 <= got < V, got
    order = rank_order(y) if order is None else order
    if temperature == 0 or top_k == 1:
        if got == order[0]:
            return True
        assert y_tol > 0 and y[order[0]] - y[got] <= y_tol, ("not the argmax", got, int(order[0]))
        return False
    mass = masses(y, temperature, f32) if mass is None else mass
    nK = V if top_k is None else min(int(top_k), V)
    k_close = nK < V and y_tol > 0 and y[order[nK - 1]] - y[order[nK]] < y_tol
    n, p_close = nK, False
    if top_p is not None and top_p < 1:
        c = np.cumsum(mass[order[:nK]])
        n = min(int(np.searchsorted(c, top_p * c[-1], side="left")) + 1, nK)
        p_close = cut_distance(mass[order[:nK]], top_p) <= tol

    def keep(n_words):
        k = np.zeros(V, dtype=bool)
        k[order[:n_words]] = True
        return k

    fit = _draw_fits(mass, keep(n), u, got, tol)
    if fit == "exact":
        return True
    if fit == "near" or k_close:
        return False
    assert p_close, ("draw %d is not the rule's" % got, int(G.inverse_cdf(np.where(keep(n), mass, 0.0), u)), bool(keep(n)[got]), n)
    assert any(1 <= n2 <= nK and _draw_fits(mass, keep(n2), u, got, tol) for n2 in (n - 1, n + 1)), ("ambiguous cut, but no fit", got, n)
    return False


def oracle_follow(lm, prompts, ids, temperature, seed, top_k, top_p, tol):
    """the oracle teacher-forced on the device's draws: -> (agreeing draws, excused draws, oracle nll per row)"""
    sn = lm.config["self_norm"]
    agree = excused = 0
    out = []
    for r, (p, x) in enumerate(zip(prompts, ids)):
        h, c = lm.zero_state(1)
        for w in p:
            h, c = lm.lstm_cell(np.array([w]), h, c)
        nll = []
        for k, w in enumerate(x):
            y = lm.project(h)[0]
            nll.append(-y[w] if sn else lse(y) - y[w])
            ok = judge_draw(y, temperature, top_k, top_p, float(G.uniform(seed, k, r)), int(w), tol, y_tol=tol, f32=False)
            agree += ok
            excused += not ok
            h, c = lm.lstm_cell(np.array([w]), h, c)
        out.append(np.array(nll))
    return agree, excused, out
