"""The derived error bars of cache_query_kernel and cache_mix_rows_kernel (csrc/jlm_cache_mix.hip), built as tests/cache_budget.py is:
nothing here is measured, every figure follows from the arithmetic the kernels use (include/jlm_hip.h states it).  u = 2^-24.

  products   a key's dot product is four f32 fmaf chains of H / 4 terms and two f32 additions: gamma_(H/4 + 2) <= gamma_H relative to
             A = sum_k |q_k| |k_k|.  Split rows are decoded as f32(hi) + f32(lo): exact unless lo is so small beside hi that the sum
             needs more than 24 bits, then within u of the value -- u on each operand of a product, 2 u (1 + u) on A.
  scores     s_j = f32(theta' * dot) (theta' = theta / h_scale^2, exact: a power of two) and the f32 difference s_j - max with
             |s_j - max| <= 2 theta A: 3 u theta A; the reference takes theta as the f32 the launcher is passed:
                 DS = theta * A * (E(H) + 4 u)
  log c, log Z   log sum exp is 1-Lipschitz in the largest |delta s_j|, once each:     2 DS
  the sums   c and Z are f32 sums of at most N positive terms, each expf within an ulp (2 u relative), at most N - 1 additions (u
             each, of positive partial sums):     ES = (2 + N) u * 1.01 on log c and on log Z each
  logf       within an ulp of its result, and the f32 subtraction:     2 u (|log c| + |log Z| + 1) + u |log c - log Z|
      LPC_BAR = 2 DS + 2 ES + 2 u (|log c| + |log Z| + 1) + u |lpc|

  L          topk_rows_kernel's arithmetic: the f32 difference y - m is within u |y - m|, which moves a term of the sum by that
             relative amount, expf by 2 u more; the sum is in f64.  On log S: sum_w p(w) (u |y_w - m| + 2 u), with p the row's
             softmax, computed by the reference.  Rounded to f32: u |L|.  (1e-12 covers the f64 operations.)
  the term   t = f32(f32(L + logf(rho)) + lpc): logf(rho) is the f64 value rounded to f32, u |log rho|; the two additions u |L +
             log rho| and u |t|.
  y'         m + log1pf(expf(d)), d = min - max: y' is 1-Lipschitz in t and in y (y is exact); d is within u |d| and log1p(exp(.))
             is 1/2-Lipschitz; expf within an ulp moves log1p by at most 2 u * 1/2; log1pf within an ulp of a value <= log 2; the
             last addition u |y'|:
      Y_BAR = LPC_BAR + L_BAR + u (|log rho| + |L + log rho| + |t|) + u |d| / 2 + 3 u + u |y'|
"""
import numpy as np

U = 2.0 ** -24


def e_products(split, H):
    """relative to A = sum_k |q_k| |k_k|: the error of one product h_q . h_i of cache_query_kernel"""
    return H * U / (1 - H * U) + (2 * U * (1 + U) if split else 0.0)


def e_sums(N):
    """relative error of each of the two f32 sums of at most N positive terms"""
    return (2 + N) * U * 1.01


def score_bar(split, H, theta, A):
    """|s_j - theta dot| of jlm_cache_query alone (no difference with the maximum): the products and the one product with theta"""
    return float(np.float32(theta)) * A * (e_products(split, H) + 2 * U)


def lpc_bar(split, H, N, theta, A, logc, logZ):
    """LPC_BAR: A = the largest sum_k |q_k| |k_k| over the window, logc / logZ the reference's two logarithms under the maximum"""
    ds = float(np.float32(theta)) * A * (e_products(split, H) + 4 * U)
    return 2 * ds + 2 * e_sums(N) + 2 * U * (abs(logc) + abs(logZ) + 1) + U * abs(logc - logZ)


def lse_bar(y, self_norm):
    """L_BAR of one row of f32 logits (float64 reference arithmetic): 0 on self-normalised models, where L = 0 exactly"""
    if self_norm:
        return 0.0
    y = np.asarray(y, dtype=np.float64)
    m = y.max()
    p = np.exp(y - m)
    S = p.sum()
    L = m + np.log(S)
    with np.errstate(invalid="ignore"):
        spread = np.where(p > 0, p * np.abs(y - m), 0.0).sum() / S
    return U * spread + 2 * U + U * abs(L) + 1e-12


def y_bar(lpc_b, L_b, L, log_rho, lpc, y, y_new):
    """Y_BAR of one patched word: lpc_b / L_b the two bars above, the other arguments the reference's values"""
    t = L + log_rho + lpc
    d = 0.0 if np.isneginf(y) else min(y, t) - max(y, t)
    return lpc_b + L_b + U * (abs(log_rho) + abs(L + log_rho) + abs(t)) + U * abs(d) / 2 + 3 * U + U * abs(y_new)
