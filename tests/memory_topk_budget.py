"""The derived error bar of a score of memory_topk_score_kernel (csrc/jlm_memory_topk.hip), shared by tests/test_gpu_memory_topk.py and
tests/test_gpu_rank_memory.py.  Nothing here is measured.

A score is s_i = f32(theta' * dot_i) + 0 with theta' = f32(theta / h_scale^2) (f32 rows: theta) and dot_i off the matrix pipe by
memory_rows_kernel's instructions in its k order.  With A_i = sum_k |q_k| |k_k| in real units and u = 2^-24:

  the product   cache_rows_kernel's term, the same instructions in the same order (tests/cache_budget.py e_products, whose derivation
                tests/test_gpu_cache_rows.py holds):                                    |delta dot_i| <= e_products(split, H) A_i
  theta'        one f32 division (exact when h_scale is a power of two):               u theta A_i
  the multiply  one f32 rounding of a value of at most theta A_i (1 + ...):             u theta A_i
  + 0           exact

  |s_i - theta (h_q . k_i)| <= theta A_i (e_products(split, H) + 2 u)                  (score_bar; theta as the f32 the launcher gets)

The selection adds nothing: it compares the bits of the scores it is given.  So an entry i that is NOT returned has a computed score at
most that of every returned j, and with bar = max_i of the bars of the row
    s64_i <= min_j s64_j + 2 bar
exactly -- condition (c) of tests/test_gpu_memory_topk.py, with no case left out.
"""
import numpy as np

from tests.cache_budget import U, e_products


def lpc_bar(split, H, n_q, theta, A, logc, logZ):
    """tests/cache_mix_budget.py LPC_BAR -- the bar of log c(w) - log Z as cache_mix_rows_kernel forms it from n_q scores -- with the
    product term above in cache_query_kernel's place: the scores' own bar and the f32 difference s_j - max (2 u theta A more) enter
    log c and log Z once each, the two f32 sums of at most n_q positive terms, the two logf and the subtraction.  A: the largest
    sum_k |q_k| |k_k| over the retrieved entries; logc / logZ: the reference's two logarithms under the maximum."""
    ds = float(np.float32(theta)) * A * (e_products(split, H) + 4 * U)
    return 2 * ds + 2 * (2 + n_q) * U * 1.01 + 2 * U * (abs(logc) + abs(logZ) + 1) + U * abs(logc - logZ)


def score_bar(split, H, theta, A):
    """the bar of one score (or an array of them): A = sum_k |q_k| |k_k| of its pair"""
    return float(np.float32(theta)) * np.asarray(A, dtype=np.float64) * (e_products(split, H) + 2 * U)
