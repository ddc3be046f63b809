"""The derived bars of a decode under a memory (tests/test_decode_memory_cpu.py, tests/test_gpu_decode_memory.py).
Nothing here is measured on the code under test: every figure follows from the arithmetic the kernels use (include/jlm_hip.h states
it), from the yardstick's own float64 states, and from bars the suite already holds.  u = 2^-24, r = 2e-6 (check_nbest's rtol).

  one score      s_i is jlm_memory_topk's: |s_i - theta (h_q . k_i)| <= theta A_i (e_products(split, H) + 2 u) over the rows it is given
                 (tests/memory_topk_budget.py score_bar), A_i = sum_k |q_k| |k_k|.
  the states     End to end the device's rows are not the oracle's.  Section 28 widens a bar by theta (|Dq . k| + |q . Dk| + |Dq . Dk|)
                 from the device's own states.  A decode's hypothesis rows are not read back, so D is bounded instead: the suite holds a
                 device state to the relative accuracy of the scores, r, and a state row comes off accumulations whose rounding is
                 relative to the row's largest element, |Dq_k| <= r |q|_inf, |Dk_k| <= r |k|_inf:
                     theta r (1 + r) (|q|_inf |k_i|_1 + |k_i|_inf |q|_1)
                 (tests/decode_cache_budget.py word_bar takes the same term at its worst case, every unit at 1: 2 r theta H).
      SCORE_BAR_i = theta A_i (e_products(split, H) + 2 u) + theta r (1 + r) (|q|_inf |k_i|_1 + |k_i|_inf |q|_1)
                 the end-to-end bar of one score against the float64 score over the ORACLE's states q, k_i, taken at the larger of the two
                 state-row formats so that the fixture does not depend on the format.  Two entries whose float64 scores differ by more
                 than the sum of their bars -- at most 2 max_i SCORE_BAR_i -- are ordered alike by the device and by the definition.
  the patch      memory_cell_patch_kernel is cache_cell_patch_kernel's arithmetic over a list of n_q = min(K, N) entries: the f32
                 difference s_i - max (2 u theta A more on a score: DS = theta A (e_products + 4 u), decode_cache_budget.ds, to which the
                 retrieval's product term is equal -- the same instructions in the same order, section 29), log M and log Z 1-Lipschitz
                 in it once each, the two f32 sums of at most n_q positive terms (ES), the rounding of edge'.
      WORD_BAR  = decode_cache_budget.word_bar at N_window = n_q     (A <= H: |h| < 1 in every unit)
                 what the memory may add to the error of one word's cost on top of what context_cases.check_nbest allows the decode
                 without it; a path of n words is held to atol 2e-5 + n WORD_BAR, rtol 2e-6.
"""
import numpy as np

from tests.cache_budget import U, e_products
from tests.decode_cache_budget import word_bar as _cache_word_bar

STATE_RTOL = 2e-6                       # check_nbest's rtol: what the suite holds a device state to against the oracle's
RTOL, ATOL = 2e-6, 2e-5                 # check_nbest's bars


def score_bars(q, keys, theta):
    """SCORE_BAR_i of every entry: q [H], keys [N, H] the oracle's float64 states -> [N] float64"""
    q, keys = np.asarray(q, dtype=np.float64), np.asarray(keys, dtype=np.float64)
    H, th, r = q.shape[0], float(np.float32(theta)), STATE_RTOL
    aq, ak = np.abs(q), np.abs(keys)
    kernel = th * (ak @ aq) * (max(e_products(True, H), e_products(False, H)) + 2 * U)
    state = th * r * (1 + r) * (aq.max() * ak.sum(axis=1) + ak.max(axis=1) * aq.sum())
    return kernel + state


def word_bar(split, H, n_q, theta):
    """WORD_BAR: what the memory may add to the error of one word's cost in a decode"""
    return _cache_word_bar(split, H, n_q, theta)


def path_atol(split, H, n_q, theta, n_words):
    """the absolute bar of a path's score: check_nbest's atol widened per word"""
    return ATOL + n_words * word_bar(split, H, n_q, theta)
