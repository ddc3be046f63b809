"""The derived error bar of ngram_mix_rows_kernel (csrc/jlm_ngram_mix.hip), built as tests/cache_mix_budget.py is: nothing here is
measured, every figure follows from the arithmetic the kernel uses (include/jlm_hip.h states it).  u = 2^-24.  The table's values are
the f32 the device holds, so q's operands are exact; the reference takes lambda as the f32 the launcher is passed.

  L          topk_rows_kernel's arithmetic, as cache_mix_rows_kernel restates it: ``cache_mix_budget.lse_bar`` (the f32 differences
             y - m, expf within an ulp, f64 sums, L rounded to f32), 0 on self-normalised models where L = 0 exactly:     L_BAR
  log rho    the f64 value rounded to f32:     u |log rho|
  base       f32(L + log rho):     u |L + log rho|
  q          a trigram successor: lp itself, exact.  A bigram successor: f32(bow(u v) + lp), u |q|.  A unigram: back = f32(bow(u v) +
             bow(v)), u |back|, then f32(back + lp), u |q| (1 + u).  For every level at most     u (|back| + |q|) * (1 + u)
  t          f32(base + q):     u |t|
  y'         m + log1pf(expf(d)), d = min - max: y' is 1-Lipschitz in t and in y (y is exact); d is within u |d| and log1p(exp(.))
             is 1/2-Lipschitz; expf within an ulp moves log1p by at most 2 u * 1/2; log1pf within an ulp of a value <= log 2; the
             last addition u |y'| (cache_mix_budget's last line, term for term):     u |d| / 2 + 3 u + u |y'|
             y = -inf: y' = t itself, and the same expression (d = 0) covers it.

      Y_BAR = L_BAR + u (|log rho| + |L + log rho| + (|back| + |q|) (1 + u) + |t|) + u |d| / 2 + 3 u + u |y'|

On top of a ranking's or a selection's own bar, a mixed logit moves by at most Y_BAR and the mixed row's lse by at most the largest
Y_BAR of the row (lse is 1-Lipschitz in the largest change): ``row_bar`` is that maximum.
"""
import numpy as np

from tests.cache_mix_budget import U, lse_bar                                             # noqa: F401


def y_bar(y, q, back, lam, self_norm, y_new):
    """Y_BAR of every word of one row, as an array [V] (0 where q = -inf: those words keep their bits).  y: the row's f32 logits, q:
    the reference's q(. | history) over the row (float64, -inf for "no unigram"), back: bow(u v) + bow(v) of the contexts in use,
    y_new: the reference's mixed logits."""
    y, q, y_new = np.asarray(y, dtype=np.float64), np.asarray(q, dtype=np.float64), np.asarray(y_new, dtype=np.float64)
    lam = float(np.float32(lam))
    log_rho = np.log(lam) - np.log1p(-lam)
    if self_norm:
        L = 0.0
    else:
        m = y.max()
        L = m + np.log(np.exp(y - m).sum())
    L_b = lse_bar(y, self_norm)
    at = np.isfinite(q)
    qq = np.where(at, q, 0.0)
    t = L + log_rho + qq
    with np.errstate(invalid="ignore"):
        d = np.where(np.isneginf(y), 0.0, np.minimum(y, t) - np.maximum(y, t))
    bar = L_b + U * (abs(log_rho) + abs(L + log_rho) + (abs(back) + np.abs(qq)) * (1 + U) + np.abs(t)) + U * np.abs(d) / 2 + 3 * U + \
        U * np.abs(np.where(at, y_new, 0.0))
    return np.where(at, bar, 0.0)


def row_bar(y, q, back, lam, self_norm, y_new):
    """the largest Y_BAR of a row: what a mixed logit, and the mixed row's lse, moves by at most"""
    return float(y_bar(y, q, back, lam, self_norm, y_new).max())
