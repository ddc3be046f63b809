"""A numpy double of the device side of the n-gram mixture (csrc/jlm_ngram_edge.hip, include/jlm_hip.h jlm_ngram_cell_patch): the
hash-table probe exactly as the kernel walks it, back-off over it, and the rewrite of one cell's edge logits in float64.  The CPU
tests hold the table format and the host-side search against it; nothing here touches a GPU."""
import numpy as np

from jlm_amd.ngram import GOLDEN, pack

MASK64 = (1 << 64) - 1


def probe(arr, key):
    """(lp, bow) of ``key`` in a device_arrays() table, or None: the home slot, then linear probing until the key, an empty slot, or
    max_probe + 1 slots"""
    log2cap, keys, vals = arr["log2cap"], arr["keys"], arr["vals"]
    slot = ((int(key) * GOLDEN) & MASK64) >> (64 - log2cap)
    for _ in range(arr["max_probe"] + 1):
        k = int(keys[slot])
        if k == int(key):
            return float(vals[slot, 0]), float(vals[slot, 1])
        if k == 0:
            return None
        slot = (slot + 1) & ((1 << log2cap) - 1)
    return None


def logq(arr, order, hist, w):
    """q(w | hist) over the hash table, as the kernel forms it: float32 table values, float64 sums"""
    k = min(order - 1, len(hist))
    h = tuple(int(x) for x in hist[len(hist) - k:]) if k else ()
    acc = 0.0
    while True:
        e = probe(arr, pack(h + (int(w),)))
        if e is not None:
            return acc + e[0]
        if not h:
            return -np.inf
        c = probe(arr, pack(h))
        if c is not None:
            acc += c[1]
        h = h[1:]


def patch_cell(arr, order, lam, hists, words, y, L):
    """edge' [len(words), len(hists)] float32 of one cell: hists the slots' histories, words the cell's word list, y [words, slots]
    float32 edge logits, L [slots] float64 log-normalisers"""
    lam = float(np.float32(lam))
    log1m, log_rho = np.log1p(-lam), np.log(lam) - np.log1p(-lam)
    out = np.empty(np.shape(y), dtype=np.float32)
    for p, w in enumerate(words):
        for k, h in enumerate(hists):
            q, yy = logq(arr, order, h, w), float(y[p][k])
            out[p, k] = L[k] + log1m + np.logaddexp(yy - L[k], log_rho + q) if np.isfinite(q) else yy + log1m
    return out
