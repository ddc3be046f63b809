"""Rows that pin the log-normaliser L of cache_mix_rows_kernel and ngram_mix_rows_kernel to topk_rows_kernel's on the device
(csrc/jlm_row_lse.h is the one definition all three call): tests/test_gpu_cache_mix_rows.py and tests/test_gpu_ngram_mix_rows.py use
them.

A row of V logits: seeded normals times 8, minus the row's maximum in f32, with the maximum moved to word p -- so y[p] = 0.0f exactly
and every other word is below it -- and one other word w* at -inf.  jlm_topk_rows with k = 1 then returns id p and
nll = (M + log S) - y[p] = M + log S, the kernel's own f64 log-normaliser.  A mix kernel that gives w* the term 0 (a unigram of
log-probability 0.0; a cache window of one entry) writes y'[w*] = logaddexp(-inf, L + log rho) = float32(L + log rho) with
L = float32(M + log S): the bits are a function of the top-k kernel's nll alone.

Widths: 5 (a single chunk), 1 030 (wave spans of 2 / 2 / 1 iterations and an empty fourth wave), 4 101 (spans of 5 / 5 / 5 / 2: a wave
runs more than one group of four chunks).  p is the first word of the first wave's span or the last word of the last non-empty
wave's.  A seed whose float64 log-normaliser is below 2^-20 is passed over: L would say nothing.

What the pin does not prove.  The mix kernels keep L as a float32, so a difference between their f64 M + log S and the top-k
kernel's below half a float32 ulp of L (about 3e-8 relative) cannot show; and at lambda = 0.5 log rho is exactly 0.0, so the expected
bits are float32(nll) and the way a kernel adds log rho is not exercised either (tests/test_gpu_cache_mix_rows.py and
tests/test_gpu_ngram_mix_rows.py hold the patched values at other lambdas to their float64 definitions)."""
import functools
import itertools

import numpy as np

from jlm_amd import _lib

WIDTHS = (5, 1030, 4101)
CASES = [(V, where) for V in WIDTHS for where in ("first", "last")]
LAM = 0.5
LOG_RHO = np.float32(np.log(np.float64(np.float32(LAM))) - np.log1p(-np.float64(np.float32(LAM))))


def wave_spans(V):
    """[(first word, end word)] of the waves that have any: 16-byte chunks, 64 chunks an iteration, four waves with contiguous spans"""
    n4 = (V + 3) // 4
    n_it = (n4 + 63) // 64
    ipw = (n_it + 3) // 4
    return [(256 * w * ipw, min(256 * min((w + 1) * ipw, n_it), V)) for w in range(4) if w * ipw < n_it]


@functools.lru_cache(maxsize=None)
def pin_row(V, where):
    """-> (y [V] float32, p, w*)"""
    spans = wave_spans(V)
    p = spans[0][0] if where == "first" else spans[-1][1] - 1
    for seed in itertools.count(1000 * V + (where == "last")):
        rng = np.random.RandomState(seed)
        y = (8.0 * rng.standard_normal(V)).astype(np.float32)
        a = int(np.argmax(y))
        if int((y == y[a]).sum()) != 1:
            continue
        y[[a, p]] = y[[p, a]]
        y = y - y[p]                                                       # float32: the maximum is 0.0 at p, every other word below it
        ws = (p + 1 + int(rng.randint(V - 1))) % V
        y[ws] = -np.inf
        assert y.dtype == np.float32 and y[p] == 0.0 and int((y >= 0.0).sum()) == 1 and ws != p
        if np.log(np.exp(y.astype(np.float64)).sum()) >= 2.0 ** -20:
            y.setflags(write=False)
            return y, p, ws


@functools.lru_cache(maxsize=None)
def topk_log_normaliser(V, where):
    """nll of jlm_topk_rows, k = 1, over a copy of the row: id p is asserted, nll is the kernel's f64 M + log S (one launch per row)"""
    import torch
    y, p, _ = pin_row(V, where)
    dev = _lib.require_gpu()
    ld = (V + 3) // 4 * 4
    yp = np.full((1, ld), np.nan, dtype=np.float32)
    yp[0, :V] = y
    yd = torch.from_numpy(yp).to(dev)
    ids = torch.full((1, 1), -7, device=dev, dtype=torch.int32)
    nll = torch.zeros((1, 1), device=dev, dtype=torch.float64)
    flags = torch.zeros(1, device=dev, dtype=torch.int32)
    torch.cuda.synchronize()
    rc = _lib.lib().jlm_topk_rows(yd.data_ptr(), ld, V, 1, 1, 0, ids.data_ptr(), nll.data_ptr(), 1, flags.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0 and int(flags.cpu()[0]) == 0 and int(ids.cpu()[0, 0]) == p, (rc, int(flags.cpu()[0]), int(ids.cpu()[0, 0]), p)
    got = float(nll.cpu()[0, 0])
    # that it IS a log-normaliser: against float64, within what f32 expf(y - m) costs the sum -- the argument's rounding, at most
    # 2^-24 |y - m| relative to a term, and expf within 2 ulp (2^-22) -- relative to S, hence absolute in log S
    fin = y[np.isfinite(y)].astype(np.float64)
    ref, bar = float(np.log(np.exp(fin).sum())), float(-fin.min()) * 2.0 ** -24 + 2.0 ** -22
    print("V %d, p in the %s span: top-k nll %.17g, float64 %.17g, |diff| %.3g, bar %.3g" % (V, where, got, ref, abs(got - ref), bar))
    assert abs(got - ref) <= bar, (V, where, got, ref, bar)
    return got


def expected_bits(V, where):
    """the u32 image of float32(float32(nll) + log rho), lambda = 0.5"""
    want = np.float32(np.float32(topk_log_normaliser(V, where)) + LOG_RHO)
    return int(np.asarray(want, dtype=np.float32).reshape(1).view(np.uint32)[0])
