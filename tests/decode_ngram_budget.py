"""The derived error bars of ngram_cell_patch_kernel (csrc/jlm_ngram_edge.hip) and of a decode under the n-gram mixture, in the style
of tests/decode_cache_budget.py: nothing here is measured, every figure follows from the arithmetic the kernel uses (include/jlm_hip.h
states it).  u = 2^-24.

  the table  lp and bow are the float32 values the table holds, on the device and in the reference alike (NGramMix keeps the rounded
             table; lam is the f32 the launcher is passed): they cost nothing.  q is a sum of at most three of them in f64.
  the rest   is float64: q, log rho, log(1 - lam), L, the logaddexp and the sums around it -- a few f64 ulps of values below 1e3 in
             magnitude: 1e-12 covers them.  y and L enter as the operands they are (y the f32 edge logit, L the f64 the fold left).
  rounding   edge' is rounded once to f32:     u |edge'|
      EDGE_BAR = u |edge'| + 1e-12                           with or without an n-gram term

End to end (tests/test_gpu_decode_ngram.py).  The mixture is a contraction in y and in L: with a = (1 - lam) exp(y - L) and
b = lam exp(q), edge' = L + log(a + b), so d edge'/dy = a / (a + b) and d edge'/dL = 1 - a / (a + b) = b / (a + b), both in [0, 1]
and summing to one.  An error of the device's y and L against the oracle's therefore reaches the word's cost L - edge' no larger than it
reaches the plain decode's cost L - y: what context_cases.check_nbest allows the decode without the mixture (rtol 2e-6, atol 2e-5 on a
path's score) carries over.  The only new term per word is the rounding above:
      WORD_BAR = u COST_MAX + 1e-12
with the cost's magnitude bounded by COST_MAX (|edge'| and |L| of a word the beam keeps are far below it on the test models).
"""
U = 2.0 ** -24
COST_MAX = 64.0


def edge_bar(edge_new):
    """EDGE_BAR of one rewritten edge logit, edge_new the reference's value"""
    return U * abs(edge_new) + 1e-12


def word_bar():
    """WORD_BAR: what the mixture may add to the error of one word's cost in a decode"""
    return U * COST_MAX + 1e-12


def score_bar(want, n_words):
    """the bar of a path's score: check_nbest's (rtol 2e-6, atol 2e-5) plus WORD_BAR per word (the path's words and <eos>)"""
    return 2e-5 + 2e-6 * abs(want) + (n_words + 1) * word_bar()
