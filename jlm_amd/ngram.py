"""A back-off word n-gram model mixed into conversion: its table, the estimator that makes one from an id
stream, the ARPA writer, and the spec ``Decoder.decode(ngram=)`` takes.

Table: tuples of 1 .. order word ids (order 1, 2 or 3) -> (lp, bow), natural logs -- lp of the conditional probability of the tuple's
last word, bow of the back-off weight of the tuple as a context (0 where the file gives none).  For a history h = (.., u, v) and a
word w, with k = min(order - 1, len(h)) history words in use::

    q(w | h_k) = lp(h_k, w)                            if (h_k, w) is in the table
               = -inf                                  else if k = 0
               = bow(h_k) [0 if absent] + q(w | h_{k-1})   else           (h_{k-1} drops the oldest word)

ARPA back-off WITH the weights (``NGramModel.predict`` keeps the reference's "longest suffix, no weights" rule, which does not sum to
one).  The mixture of a decode, per hypothesis with log-normaliser L and logit y of the word::

    p(w) = (1 - lam) exp(y - L) + lam exp(q(w | hist)),     hist = [<eos>] + context + the path's words so far

The device holds the table as an open-addressing hash table (``NGramTable.device_arrays``): key = (w + 1) | (v + 1) << 21 |
(u + 1) << 42 with the predicted word lowest and absent positions 0 (key 0: empty), home slot (key * 0x9E3779B97F4A7C15) >>
(64 - log2cap), linear probing, values float32 (lp, bow).  csrc/jlm_ngram_edge.hip reads it.

Command line::

    python -m jlm_amd.ngram --root R --vocab_size V --order 3 [--discount 0.75] [--corpus data/train.txt] [--out data/lm3]

counts the corpus and writes the file ``NGramModel`` / ``NGramDecoder`` (``python -m jlm_amd.eval -ng True``) and this module read.
"""
import math
import os

import numpy as np

MAX_ID = (1 << 21) - 2                   # word ids are packed in 21 bits as id + 1
MAX_ORDER = 3
GOLDEN = 0x9E3779B97F4A7C15
LN10 = math.log(10.0)
_SENTENCE_MARKS = ("<s>", "</s>", "<eos>")


def pack(ids):
    """the key of a tuple of 1 .. 3 word ids (Python int): the last word lowest"""
    key = 0
    for sh, w in zip((0, 21, 42), reversed(ids)):
        key |= (int(w) + 1) << sh
    return key


def _pack_cols(cols):
    """keys of n-grams given as equally long int64 columns, oldest word first"""
    key = np.zeros(cols[0].shape, dtype=np.int64)
    for sh, c in zip((0, 21, 42), reversed(cols)):
        key |= (c.astype(np.int64) + 1) << sh
    return key


class NGramTable:
    """``keys``: the packed n-grams ascending (int64; every key < 2^63), ``lp`` / ``bow`` float64 beside them.  ValueError for an
    order outside 1 .. 3, an id above 2^21 - 2, lp > 0 or a value that is not finite."""

    def __init__(self, keys, lp, bow, order):
        keys = np.asarray(keys, dtype=np.int64).reshape(-1)
        lp, bow = np.asarray(lp, dtype=np.float64).reshape(-1), np.asarray(bow, dtype=np.float64).reshape(-1)
        if int(order) not in (1, 2, 3):
            raise ValueError("an n-gram table has order 1, 2 or 3 (got %r)" % (order,))
        if not (keys.shape == lp.shape == bow.shape):
            raise ValueError("keys, lp and bow of an n-gram table are equally long")
        if keys.size and (keys.min() <= 0 or (np.diff(np.sort(keys)) == 0).any()):
            raise ValueError("the keys of an n-gram table are positive and distinct")
        if keys.size and int(keys.max()) >> (21 * int(order)):
            raise ValueError("an n-gram longer than the table's order")
        if not (np.isfinite(lp).all() and np.isfinite(bow).all()) or (lp > 0).any():
            raise ValueError("an n-gram table holds finite values and lp <= 0")
        at = np.argsort(keys, kind="stable")
        self.keys, self.lp, self.bow, self.order = keys[at], lp[at], bow[at], int(order)
        self._dev = {}                   # device -> (keys, vals) tensors (jlm_amd/engine.py), made once
        self._arrays = {}
        self._succ = {}                  # V -> successor_arrays(V)
        self._max_id = None

    def __len__(self):
        return int(self.keys.shape[0])

    @property
    def max_id(self):
        """the largest word id of any n-gram (-1: an empty table); found once -- every call under the mixture asks (check_mix)"""
        if self._max_id is None:
            self._max_id = int(max(((self.keys >> sh) & 0x1FFFFF).max() for sh in (0, 21, 42))) - 1 if len(self) else -1
        return self._max_id

    def rounded(self):
        """the table the device holds: every value the float32 nearest to it (what ``from_srilm`` returns is rounded already)"""
        lp, bow = self.lp.astype(np.float32).astype(np.float64), self.bow.astype(np.float32).astype(np.float64)
        if np.array_equal(lp, self.lp) and np.array_equal(bow, self.bow):
            return self
        return NGramTable(self.keys, lp, bow, self.order)

    # ---------------------------------------------------------------------------------------------- the float64 definition
    def _find(self, key):
        i = int(np.searchsorted(self.keys, key))
        return i if i < self.keys.shape[0] and int(self.keys[i]) == key else -1

    def entry(self, ids):
        """(lp, bow) of a tuple of word ids, or None"""
        i = self._find(pack(ids))
        return None if i < 0 else (float(self.lp[i]), float(self.bow[i]))

    def context(self, history_ids):
        """the k = min(order - 1, len) last words of a history, as a tuple"""
        k = min(self.order - 1, len(history_ids))
        return tuple(int(x) for x in history_ids[len(history_ids) - k:]) if k else ()

    def logq(self, history_ids, w):
        """q(w | history) in float64; -inf for a word without a unigram"""
        h, acc, w = self.context(history_ids), 0.0, int(w)
        if not 0 <= w <= MAX_ID:
            return -math.inf
        while True:
            i = self._find(pack(h + (w,)))
            if i >= 0:
                return acc + float(self.lp[i])
            if not h:
                return -math.inf
            j = self._find(pack(h))
            if j >= 0:
                acc += float(self.bow[j])
            h = h[1:]

    def logq_all(self, history_ids, V):
        """q(w | history) for w = 0 .. V - 1 as a float64 array (the same arithmetic as :meth:`logq`, word by word)"""
        h = self.context(history_ids)
        out = np.full(V, -np.inf)
        todo = np.ones(V, dtype=bool)
        acc = 0.0
        w = np.arange(V, dtype=np.int64)
        while True:
            key = w + 1
            for sh, x in zip((21, 42), reversed(h)):
                key = key | ((int(x) + 1) << sh)
            i = np.minimum(np.searchsorted(self.keys, key), max(len(self) - 1, 0))
            hit = todo & (self.keys[i] == key) if len(self) else np.zeros(V, dtype=bool)
            out[hit] = acc + self.lp[i[hit]]
            todo &= ~hit
            if not h:
                return out
            j = self._find(pack(h))
            if j >= 0:
                acc += float(self.bow[j])
            h = h[1:]

    # ---------------------------------------------------------------------------------------------- the device's hash table
    def device_arrays(self, min_log2cap=None, log2cap=None):
        """-> dict(keys uint64 [2^log2cap], vals float32 [2^log2cap, 2], log2cap, max_probe): capacity the smallest power of two >=
        2 x entries and at least 64 (``min_log2cap``: at least that; ``log2cap``: exactly that, ValueError when the entries do not
        fit), insertion in ascending key order -- the bytes are deterministic --, ``max_probe`` the longest displacement used."""
        memo = (min_log2cap, log2cap)
        if memo in self._arrays:
            return self._arrays[memo]
        n = len(self)
        if log2cap is None:
            log2cap = 6
            while (1 << log2cap) < 2 * n:
                log2cap += 1
            log2cap = max(log2cap, int(min_log2cap or 0))
        log2cap = int(log2cap)
        if not 6 <= log2cap <= 31 or n >= (1 << log2cap):
            raise ValueError("log2cap is 6 .. 31 and the table keeps an empty slot (%d entries, log2cap %d)" % (n, log2cap))
        cap, mask = 1 << log2cap, (1 << log2cap) - 1
        home = ((self.keys.astype(np.uint64) * np.uint64(GOLDEN)) >> np.uint64(64 - log2cap)).astype(np.int64).tolist()
        slot_of, used, max_probe = [0] * n, bytearray(cap), 0
        for i, s in enumerate(home):
            d = 0
            while used[s]:
                s = (s + 1) & mask
                d += 1
            used[s] = 1
            slot_of[i] = s
            if d > max_probe:
                max_probe = d
        keys = np.zeros(cap, dtype=np.uint64)
        vals = np.zeros((cap, 2), dtype=np.float32)
        at = np.asarray(slot_of, dtype=np.int64)
        keys[at] = self.keys.astype(np.uint64)
        vals[at, 0], vals[at, 1] = self.lp.astype(np.float32), self.bow.astype(np.float32)
        out = dict(keys=keys, vals=vals, log2cap=log2cap, max_probe=int(max_probe))
        self._arrays[memo] = out
        return out

    # ---------------------------------------------------------------------------------------------- the row walk's arrays
    def successor_arrays(self, V):
        """The layout csrc/jlm_ngram_mix.hip walks to form q(. | history) over ALL V words of a row, float32
        values, made once per V:

        ``uni_lp`` [V] (-inf without a unigram), ``uni_bow`` [V] (0 where absent); the bigrams in CSR by context word, in the table's
        ascending key order: ``bi_off`` int32 [V + 1], ``bi_w`` int32, ``bi_lp``, ``bi_bow`` (bow(v w), 0 where absent); the trigrams
        in CSR by distinct context (u, v): ``tri_off`` int32 [n_ctx + 1], ``tri_w`` int32, ``tri_lp``, and ``tri_bow`` [n_ctx] =
        bow(u v).  A context is every (u, v) that has a trigram successor or is a bigram with a back-off weight other than 0, so a
        weight without successors is found as one with them.  ``ctx_keys`` uint64 / ``ctx_vals`` int32 [2^log2cap]: the map from
        (v + 1) | (u + 1) << 21 to the context's index in :meth:`device_arrays`' scheme (the same hash, linear probing, insertion
        in ascending key order, ``max_probe`` the longest displacement); an empty slot holds key 0.  The bytes are deterministic.
        ValueError for a word id >= V."""
        V = int(V)
        if V in self._succ:
            return self._succ[V]
        if not 1 <= V <= MAX_ID + 1:
            raise ValueError("V is 1 .. %d" % (MAX_ID + 1))
        if self.max_id >= V:
            raise ValueError("the n-gram table holds word id %d, the row walk was asked for %d words" % (self.max_id, V))
        f32, M = np.float32, (1 << 21) - 1
        n1, n2 = np.searchsorted(self.keys, [1 << 21, 1 << 42])
        uni_lp, uni_bow = np.full(V, -np.inf, dtype=f32), np.zeros(V, dtype=f32)
        w1 = self.keys[:n1] - 1
        uni_lp[w1], uni_bow[w1] = self.lp[:n1].astype(f32), self.bow[:n1].astype(f32)
        k2, k3 = self.keys[n1:n2], self.keys[n2:]
        bi_off = np.zeros(V + 1, dtype=np.int64)
        np.cumsum(np.bincount((k2 >> 21) - 1, minlength=V), out=bi_off[1:])
        weighted = k2[self.bow[n1:n2] != 0.0]
        ctx = np.union1d(k3 >> 21, weighted)                               # ascending, distinct
        tri_off = np.zeros(ctx.size + 1, dtype=np.int64)
        np.cumsum(np.bincount(np.searchsorted(ctx, k3 >> 21), minlength=ctx.size), out=tri_off[1:])
        tri_bow = np.zeros(ctx.size, dtype=f32)
        at = np.searchsorted(k2, ctx)
        has = (at < k2.size) & (k2[np.minimum(at, max(k2.size - 1, 0))] == ctx) if k2.size else np.zeros(ctx.size, dtype=bool)
        tri_bow[has] = self.bow[n1:n2][at[has]].astype(f32)
        log2cap = 6
        while (1 << log2cap) < 2 * ctx.size:
            log2cap += 1
        cap, mask = 1 << log2cap, (1 << log2cap) - 1
        home = ((ctx.astype(np.uint64) * np.uint64(GOLDEN)) >> np.uint64(64 - log2cap)).astype(np.int64).tolist()
        used, slot_of, max_probe = bytearray(cap), [0] * ctx.size, 0
        for i, s in enumerate(home):
            d = 0
            while used[s]:
                s = (s + 1) & mask
                d += 1
            used[s] = 1
            slot_of[i] = s
            max_probe = max(max_probe, d)
        ctx_keys, ctx_vals = np.zeros(cap, dtype=np.uint64), np.zeros(cap, dtype=np.int32)
        at = np.asarray(slot_of, dtype=np.int64)
        ctx_keys[at], ctx_vals[at] = ctx.astype(np.uint64), np.arange(ctx.size, dtype=np.int32)
        out = dict(V=V, uni_lp=uni_lp, uni_bow=uni_bow, bi_off=bi_off.astype(np.int32), bi_w=((k2 & M) - 1).astype(np.int32),
                   bi_lp=self.lp[n1:n2].astype(f32), bi_bow=self.bow[n1:n2].astype(f32), tri_off=tri_off.astype(np.int32),
                   tri_w=((k3 & M) - 1).astype(np.int32), tri_lp=self.lp[n2:].astype(f32), tri_bow=tri_bow, ctx_keys=ctx_keys,
                   ctx_vals=ctx_vals, log2cap=log2cap, max_probe=int(max_probe), n_ctx=int(ctx.size))
        self._succ[V] = out
        return out

    # ---------------------------------------------------------------------------------------------- the file
    @classmethod
    def from_srilm(cls, path, w2i, order=3):
        """The tab-separated SRILM text ``NGramModel.parse_srilm`` reads.  n-grams with a word outside ``w2i`` or longer than
        ``order`` are dropped; ``<s>`` and ``</s>`` both mean ``<eos>``: of a merged entry lp comes from the form whose last word is
        ``</s>`` or ``<eos>`` (SRILM's -99 on ``<s>`` is a placeholder), bow from whichever form carries one."""
        if int(order) not in (1, 2, 3):
            raise ValueError("an n-gram table has order 1, 2 or 3 (got %r)" % (order,))
        table = {}                       # key -> [lp, bow, lp is from the closing form]
        with open(path, "r", encoding="utf-8") as f:
            for line in f:
                fields = line.rstrip("\n").split("\t", 2)
                if len(fields) < 2:
                    continue
                words = fields[1].split(" ")
                if not 1 <= len(words) <= int(order):
                    continue
                try:
                    ids = [w2i["<eos>" if w in _SENTENCE_MARKS else w] for w in words]
                except KeyError:
                    continue
                if max(ids) > MAX_ID or min(ids) < 0:
                    raise ValueError("a word id of an n-gram table is at most %d" % MAX_ID)
                lp = float(np.float32(LN10 * float(fields[0])))
                bow = float(np.float32(LN10 * float(fields[2]))) if len(fields) > 2 and fields[2].strip() else None
                closing = words[-1] != "<s>"
                e = table.setdefault(pack(ids), [lp, None, closing])
                if closing or not e[2]:
                    e[0], e[2] = lp, closing
                if bow is not None:
                    e[1] = bow
        keys = sorted(table)
        return cls(keys, [table[k][0] for k in keys], [table[k][1] or 0.0 for k in keys], order)


def write_srilm(table, path, i2w):
    """ARPA text with tab-separated fields (log10 values): what ``NGramModel.parse_srilm`` and ``NGramTable.from_srilm`` read.
    ``<eos>`` is written as ``</s>`` where it ends an n-gram of more than one word and as ``<s>`` elsewhere inside one; the unigram is
    written as ``</s>``."""
    by_len = {1: [], 2: [], 3: []}
    for key, lp, bow in zip(table.keys.tolist(), table.lp.tolist(), table.bow.tolist()):
        ids = [((key >> sh) & 0x1FFFFF) - 1 for sh in (42, 21, 0)]
        ids = [x for x in ids if x >= 0]
        words = [i2w[x] for x in ids]
        words = [("</s>" if (i == len(words) - 1) else "<s>") if w == "<eos>" else w for i, w in enumerate(words)]
        by_len[len(ids)].append((words, lp, bow))
    with open(path, "w", encoding="utf-8") as f:
        f.write("\n\\data\\\n")
        for n in (1, 2, 3):
            if n <= table.order:
                f.write("ngram %d=%d\n" % (n, len(by_len[n])))
        for n in (1, 2, 3):
            if n > table.order:
                continue
            f.write("\n\\%d-grams:\n" % n)
            for words, lp, bow in by_len[n]:
                line = "%s\t%s" % (repr(lp / LN10), " ".join(words))
                if bow != 0.0:
                    line += "\t%s" % repr(bow / LN10)
                f.write(line + "\n")
        f.write("\n\\end\\\n")


def estimate(ids, V, order=3, discount=0.75, eos=1):
    """An :class:`NGramTable` (float64 values, not yet rounded) from the id stream the trainer reads: sentences, each ending in
    ``eos``.  Absolute discounting in back-off form: unigrams (c(w) + 1) / (N + V) over all V ids, higher orders (c(hw) - D) / c(h)
    for seen n-grams with c(h) the sum of c(hw), bow(h) = (1 - sum_seen p(w | h)) / (1 - sum_seen p(w | h')).  The stream is read
    behind one ``eos``; no n-gram reaches across a sentence boundary (an ``eos`` stands only at the ends of one).  For every history,
    sum_w exp(q(w | h)) = 1."""
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    V, order, D = int(V), int(order), float(discount)
    if order not in (1, 2, 3):
        raise ValueError("an n-gram table has order 1, 2 or 3 (got %r)" % (order,))
    if not 1 <= V <= MAX_ID + 1:
        raise ValueError("V is 1 .. %d" % (MAX_ID + 1))
    if not 0.0 < D < 1.0:
        raise ValueError("the discount lies in (0, 1)")
    if ids.size and (ids.min() < 0 or ids.max() >= V):
        raise ValueError("the id stream holds an id outside [0, V)")
    c1 = np.bincount(ids, minlength=V).astype(np.float64)
    p1 = (c1 + 1.0) / (float(ids.size) + V)
    keys, lps, bows = [np.arange(1, V + 1, dtype=np.int64)], [np.log(p1)], [np.zeros(V)]
    s = np.concatenate(([eos], ids))
    # q of the order below, for the n-grams of this order (their suffix is seen whenever they are): a look-up by key
    low_keys, low_p = keys[0], p1
    for n in range(2, order + 1):
        if s.size < n:
            break
        cols = [s[i:s.size - n + 1 + i] for i in range(n)]
        inside = np.ones(cols[0].shape, dtype=bool)
        for c in cols[1:-1]:
            inside &= c != eos
        cols = [c[inside] for c in cols]
        if not cols[0].size:
            break
        gram, cnt = np.unique(_pack_cols(cols), return_counts=True)
        ctx = gram >> 21
        ctx_keys, inv = np.unique(ctx, return_inverse=True)
        c_h = np.bincount(inv, weights=cnt.astype(np.float64))
        p = (cnt - D) / c_h[inv]
        mask = (1 << (21 * (n - 1))) - 1
        low = low_p[np.searchsorted(low_keys, gram & mask)]
        den = 1.0 - np.bincount(inv, weights=low)
        num = 1.0 - np.bincount(inv, weights=p)
        if (den <= 0).any() or (num <= 0).any():
            raise ValueError("a context was followed by every word of the vocabulary: no mass is left to back off with")
        # bow of the contexts: entries of the order below (every context is an n-gram of it: seen with its last word)
        at = np.searchsorted(low_keys, ctx_keys)
        assert (low_keys[at] == ctx_keys).all()
        bows[-1][at] = np.log(num / den)
        keys.append(gram)
        lps.append(np.log(p))
        bows.append(np.zeros(gram.shape))
        low_keys, low_p = gram, p
    return NGramTable(np.concatenate(keys), np.minimum(np.concatenate(lps), 0.0), np.concatenate(bows), order)


class NGramMix:
    """What ``Decoder.decode(ngram=)`` takes: a table and the weight lam of its distribution, 0 < lam < 1.  ``table`` is the ROUNDED
    table -- the float32 values the device holds -- so the float64 definition over ``mix.table`` is what the kernel approximates."""

    def __init__(self, table, lam):
        if not isinstance(table, NGramTable):
            raise ValueError("NGramMix takes an NGramTable (got %r)" % (type(table).__name__,))
        lam = float(lam)
        if not 0.0 < lam < 1.0:
            raise ValueError("the weight of the n-gram model lies in (0, 1) (got %r)" % (lam,))
        self.table, self.lam = table.rounded(), lam

    def host_mixer(self, history_ids, V):
        """mix(pred [V]) -> (1 - lam) pred + lam exp(q(. | history)) in float64"""
        q = np.exp(self.table.logq_all(history_ids, V))
        return lambda pred: (1.0 - self.lam) * np.asarray(pred, dtype=np.float64) + self.lam * q


def check_mix(ngram, V=None):
    """the ``ngram=`` of a decode: an :class:`NGramMix` whose ids lie below the model's V; ValueError otherwise"""
    if not isinstance(ngram, NGramMix):
        raise ValueError("ngram must be an NGramMix (got %r)" % (ngram,))
    if V is not None and ngram.table.max_id >= int(V):
        raise ValueError("the n-gram table holds word id %d, the model has %d words" % (ngram.table.max_id, int(V)))
    return ngram


def mixture_nll(nll, logq, lam):
    """-log((1 - lam) exp(-nll) + lam exp(logq)) elementwise in float64 (the host form of the mixture's perplexity)"""
    nll, logq = np.asarray(nll, dtype=np.float64), np.asarray(logq, dtype=np.float64)
    return -np.logaddexp(math.log1p(-lam) - nll, math.log(lam) + logq)


def mixed_logits(table, history, y, lam, self_norm=False):
    """The logits of the mixture (1 - lam) p_lm + lam exp(q(. | history)) over a whole row, in float64: with
    L = lse(y), or 0 on self-normalised models, and rho = lam / (1 - lam),

        y'[w] = logaddexp(y[w], L + log rho + q(w | history))     where q is finite (y[w] = -inf gives the finite n-gram term)
        y'[w] = y[w]                                              where q = -inf

    so that (1 - lam) exp(y' - L) is the mixture.  ``history``: the word ids before the row's word, oldest first (``table.context``
    takes the last order - 1 of them); ``table`` holds the float32 values the device holds (``NGramMix.table``).  On ordinary models
    the selection kernels report lse(y') - y'[w]: -log of the ROW-NORMALISED mixture p_mix(w) / ((1 - lam) + lam Z_h), Z_h = sum_w
    exp q(w | h).  That is p_mix itself for a table that sums to one, as ``estimate``'s do; for a file whose out-of-vocabulary
    n-grams were dropped it differs by a constant per row.  On self-normalised models they report -y', and the host adds
    -log1p(-lam)."""
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    lam = float(lam)
    if not 0.0 < lam < 1.0:
        raise ValueError("the weight of the n-gram model lies in (0, 1) (got %r)" % (lam,))
    history = [int(x) for x in history]
    gaps = [i for i, x in enumerate(history) if x < 0]
    if gaps:                                                               # -1: no word there, and none before it
        history = history[gaps[-1] + 1:]
    q = table.logq_all(history, y.shape[0])
    if self_norm:
        L = 0.0
    else:
        m = y.max()
        L = m + math.log(np.exp(y - m).sum())
    out = y.copy()
    at = np.isfinite(q)
    out[at] = np.logaddexp(y[at], L + (math.log(lam) - math.log1p(-lam)) + q[at])
    return out


SUCCESSOR_TENSORS = ("uni_lp", "uni_bow", "bi_off", "bi_w", "bi_lp", "tri_off", "tri_w", "tri_lp", "tri_bow", "ctx_keys", "ctx_vals")
MIX_MAX_V = 393216                       # JLM_NGRAM_MIX_MAX_V (include/jlm_hip.h): the patched-word bitmap of a row takes 48 KB of LDS


def successor_tensors(table, V, device):
    """-> (dict of the device tensors of ``table.successor_arrays(V)`` in the order of SUCCESSOR_TENSORS -- ctx_keys as int64 --, the
    arrays), made once per (table, V, device) and kept beside ``DecodeEngine.ngram_tensors``' on the table"""
    import torch
    key = ("rows", int(V), device.type, device.index)
    if key not in table._dev:
        arr = table.successor_arrays(V)
        # (an empty list is uploaded as one zero: the launcher refuses a null pointer, the lengths travel beside the tensors)
        up = lambda a: torch.from_numpy((a.view(np.int64) if a.dtype == np.uint64 else a) if a.size else np.zeros(1, a.dtype)).to(device)
        table._dev[key] = ({name: up(arr[name]) for name in SUCCESSOR_TENSORS}, arr)
    return table._dev[key]


def check_mix_rows(ngram, V):
    """``check_mix`` for a call that patches whole rows: also ValueError for a vocabulary whose bitmap the kernel cannot hold"""
    check_mix(ngram, V)
    if int(V) > MIX_MAX_V:
        raise ValueError("the n-gram mixture over whole rows takes at most %d words (the model has %d)" % (MIX_MAX_V, int(V)))
    return ngram


def stream_logq(table, ids, eos=1):
    """q(ids[t] | [eos] + ids[:t]) for every position of an id stream, float64"""
    s = [int(eos)] + [int(x) for x in np.asarray(ids).reshape(-1)]
    return np.array([table.logq(s[max(0, t - 2):t], s[t]) for t in range(1, len(s))], dtype=np.float64)


def main(argv=None):
    import argparse
    from . import config as _config
    from .data import Vocab
    from .perplexity import encode_lines, read_lines
    ap = argparse.ArgumentParser(prog="python -m jlm_amd.ngram", description="count a corpus into a back-off n-gram file (ARPA text)")
    ap.add_argument("--root", default=None)
    ap.add_argument("--vocab_size", type=int, required=True)
    ap.add_argument("--order", type=int, default=3)
    ap.add_argument("--discount", type=float, default=0.75)
    ap.add_argument("--corpus", default=os.path.join("data", "train.txt"))
    ap.add_argument("--out", default=os.path.join("data", "lm3"))
    args = ap.parse_args(argv)
    if args.root:
        _config.set_root(args.root)
    base = os.path.dirname(os.path.normpath(_config.data_path))
    at = lambda p: p if os.path.isabs(p) else os.path.join(base, p)
    vocab = Vocab(args.vocab_size)
    sents, n_unk = encode_lines(read_lines(at(args.corpus)), vocab)
    ids = np.array([i for s in sents for i in s], dtype=np.int64)
    table = estimate(ids, len(vocab), args.order, args.discount, eos=vocab.w2i["<eos>"]).rounded()
    write_srilm(table, at(args.out), vocab.i2w)
    print("%d sentences, %d tokens (%d <unk>) -> %d n-grams of order <= %d in %s" % (
        len(sents), ids.size, n_unk, len(table), args.order, at(args.out)))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
