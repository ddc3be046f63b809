"""The derived error bars of cache_cell_query_kernel and cache_cell_patch_kernel (csrc/jlm_cache_edge.hip), in the style of
tests/cache_mix_budget.py: nothing here is measured, every figure follows from the arithmetic the kernels use (include/jlm_hip.h states
it).  u = 2^-24.

  scores     s is jlm_cache_query's, bit for bit: cache_mix_budget.score_bar; with the f32 difference s_i - max (|s_i - max| <= 2 theta
             A), as there:     DS = theta A (E(H) + 4 u)
  log M, log Z   log sum exp is 1-Lipschitz in the largest |delta s_i|, once each:     2 DS
  the sums   M and Z are f32 sums of at most N positive terms, each expf within an ulp (2 u relative), at most N - 1 additions:
             ES = (2 + N) u 1.01 on log M and on log Z each (cache_mix_budget.e_sums)
  the rest   is float64: log M, log Z, log rho, log(1 - lam), L, the logaddexp and the sums around it -- 1e-12 covers them; lam is the f32
             the launcher is passed (the reference takes that value).  y and L enter as the operands they are (y the f32 edge logit, L
             the f64 the fold left), so they cost nothing here; edge' is 1-Lipschitz in log M - log Z (the mixture's derivative with
             respect to log c is lam c / p <= 1).
  rounding   edge' is rounded once to f32:     u |edge'|
      EDGE_BAR = 2 DS + 2 ES + u |edge'| + 1e-12             for a word with a match
      EDGE_BAR = u |edge'| + 1e-12                           for a word without (y + log(1 - lam) in f64, rounded once)

End to end (tests/test_gpu_decode_cache.py) a path's score adds, per word, the cache's share of that word's cost on top of what
context_cases.check_nbest allows the decode without a cache: WORD_BAR = 2 DS + 2 ES + u |cost| with A <= H (|h| < 1 in every unit: h
= o tanh(c)) -- the edge logit's own rounding and L's error are in check_nbest's bars already, the cost's magnitude is bounded by
COST_MAX below.
"""
import numpy as np

from tests.cache_mix_budget import U, e_products, e_sums

COST_MAX = 64.0                         # |edge'| of a word the beam keeps: -log p of a path word is far below this on the test models


def ds(split, H, theta, A):
    return float(np.float32(theta)) * A * (e_products(split, H) + 4 * U)


def edge_bar(split, H, N, theta, A, edge_new, match, spread=None):
    """EDGE_BAR of one rewritten edge logit: A = the largest sum_k |q_k| |k_k| over the slot's window, edge_new the reference's value.
    spread: the scores are GIVEN (a test of the patch alone) -- DS is the f32 difference s_i - max alone, u max |s_i - max|"""
    if not match:
        return U * abs(edge_new) + 1e-12
    d = ds(split, H, theta, A) if spread is None else U * spread
    return 2 * d + 2 * e_sums(N) + U * abs(edge_new) + 1e-12


def word_bar(split, H, N, theta):
    """WORD_BAR: what the cache may add to the error of one word's cost in a decode (A <= H).  The device's states are not the
    oracle's: they are held to the relative accuracy the scores are (check_nbest's rtol, 2e-6), on the query and on the key."""
    return 2 * (ds(split, H, theta, float(H)) + 2 * 2e-6 * float(np.float32(theta)) * H) + 2 * e_sums(N) + U * COST_MAX
