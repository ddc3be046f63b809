"""Where the word that was actually written ranks, on the device: ``LSTM_Model.rank`` / ``rank_streams`` and the figures of a
predictive keyboard that follow from the ranks.

The reference has ``find_top_N`` over one host-side distribution (decoder/model.py:25-26) and nothing that measures how good a
candidate list is on a corpus.  Here a call is ONE op (``torch.ops.jlm.rank_frames``, csrc/jlm_decode.hip ``jlm_rank_frames``): per
step the LSTM step and the T projection of the live rows as ``score`` launches them, the full-vocabulary logits as ``generate``
materialises them (``jlm_gemm_nt`` per segment), and ``rank_rows_kernel`` (csrc/jlm_rank.hip), which counts the words that rank above
the step's target.  Nothing comes back to the host between steps.

Definitions (include/jlm_hip.h jlm_rank_rows; pinned by tests/test_rank_cpu.py and tests/test_gpu_rank_rows.py).  For a row of logits
y, its target t and a set S of word ids, the 0-based

    rank(S) = #{ w in S : y[w] > y[t] } + #{ w in S : w < t and y[w] == y[t] }

-- ``predict_top``'s order: logit descending, lower id first on a tie.  The log-normaliser does not enter.  The levels of a target
whose katakana reading r has n kana (``ReadingIndex.level_table``):

    A    every word;
    j    for j = 0 .. min(n, max_prefix): the words whose reading starts with r[:j] -- what ``predict_reading`` ranks after j typed kana
         (j = 0: every word that has a reading);
    X    the words whose reading equals r: its homophones, the position in a conversion candidate window.

A word without a reading (``<eos>``, ``<unk>``) has level A only; a level a target does not have holds -1.  The result columns are
A, the prefix levels 0 .. max_prefix, then X: ``max_prefix + 3`` of them (``readings=False``: column A alone).

The metrics at the end of this module are plain numpy over such arrays.
"""
import numpy as np

from . import ops as _ops
from . import rowsets
from .cache import MixRings
from .generate import GENERATE_BUDGET_BYTES, MAX_ROWS
from .rowsets import RowSets, check_streams, forced_rows
from .score import sentence_loop

MAX_PREFIX_LIMIT = 30               # prefix levels 0 .. 30 and level X: the 32 level columns of jlm_rank_rows


def check_max_prefix(max_prefix):
    if not rowsets.is_int(max_prefix) or not 0 <= max_prefix <= MAX_PREFIX_LIMIT:
        raise ValueError("max_prefix must be an integer in [0, %d] (got %r)" % (MAX_PREFIX_LIMIT, max_prefix))
    return int(max_prefix)


class Levels:
    """The level table of one (ReadingIndex, max_prefix) on the device: ids, the CSR (off, lo, hi), and its host copy of off."""

    def __init__(self, m, index, max_prefix):
        torch = m.torch
        self.index, self.max_prefix = index, max_prefix
        self.n_levels = max_prefix + 2
        if index.V != m.V:
            raise ValueError("the reading index covers %d words, the model %d" % (index.V, m.V))
        off, lo, hi = index.level_table(max_prefix)
        self.off_host = off
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(m.device)
        self.ids, self.off, self.lo, self.hi = up(index.ids), up(off), up(lo), up(hi)

    def args(self):
        return self.ids, self.off, self.lo, self.hi, self.n_levels

    def to_columns(self, dev_rank, target):
        """device ranks [N, n_levels + 1] of the targets [N] -> the public columns: level X moved from behind the target's prefix
        levels to the last column"""
        out = dev_rank.copy()
        t = np.asarray(target, dtype=np.int64)
        cnt = (self.off_host[t + 1] - self.off_host[t]).astype(np.int64)          # 0, or the prefix levels + 1
        has = np.flatnonzero((cnt > 0) & (cnt < self.n_levels))
        out[has, self.n_levels] = dev_rank[has, cnt[has]]
        out[has, cnt[has]] = -1
        return out


class Ranker:
    """The device side of a ranking call over a :class:`jlm_amd.model.DeviceModel`."""

    def __init__(self, dev_model):
        self.m = dev_model
        self.torch = dev_model.torch
        self.last_step_ms = None          # [n_steps, 4] of the last timed call: LSTM step, T projection, logit GEMMs, ranking
        self._levels = {}

    def levels(self, index, max_prefix):
        """the uploaded level table of (index, max_prefix), made on first use"""
        key = (id(index), int(max_prefix))
        if key not in self._levels:
            with self.m._ctx():
                self._levels[key] = Levels(self.m, index, int(max_prefix))
        return self._levels[key]

    def row_bytes(self, n_steps, n_levels, cache_size=0, top=0, ngram=False):
        """the bytes a row of a call takes; ``cache_size`` > 0: with the rings and the score scratch of a cached call; ``ngram``: with
        the histories [n_steps, 2] int32 (and ``top`` lists) of a call under the n-gram mixture"""
        m = self.m
        base = (rowsets.ld_logits(m.V) + 4 * m.H + m.ldt) * 4 + n_steps * (8 + 4 * (n_levels + 1)) + 32
        if cache_size:
            base += MixRings.row_bytes(m.H, cache_size, n_steps, top)
        if ngram:
            base += n_steps * (8 + 12 * top)
        return base

    def run(self, word, target, n_live, h=None, c=None, levels=None, timed=False, rings=None):
        """One call: word / target [n_steps, R] int32 (host), n_live [n_steps] (host; non-increasing, rows live as a prefix).  h, c:
        the state to continue ([R, H] device tensors in the model's state-row format, as returned here), None = the zero state.
        levels: a :class:`Levels`, None = level A only.  rings: a :class:`jlm_amd.cache.MixRings` made for this call's (R, n_steps) --
        the op is then ``rank_cache_frames``: every step's logits are patched into the mixed distribution of the continuous cache
        before they are ranked, the rings' ``top`` best words of every step go to the rings' lists, and last_step_ms has six columns
        (the cache's query and patch between the logit GEMMs and the ranking); a :class:`jlm_amd.ngram_mix.NgramPatch`: the op is
        ``rank_ngram_frames``, the patch is the n-gram mixture's and last_step_ms has five columns.  -> (rank [n_steps, R, n_levels + 1] int32 in the device's column order, -1
        where a row is not live, h, c) -- the state after the last step stays on the device; as in Scorer.run, only the rows live
        at the last step are defined in it."""
        torch, m = self.torch, self.m
        L = levels.n_levels if levels is not None else 0
        with m._ctx():
            rs = RowSets(m, np.shape(target)[1], logits=True)
            S, R, forced = forced_rows(m, rs, word, target, n_live, h, c, "rank")
            rank = torch.full((S, R, L + 1), -1, device=m.device, dtype=torch.int32)
            table = levels.args() if levels is not None else (None, None, None, None, 0)
            args = (m.decode_model(), *rs.state(), rs.logits, rs.ld_logits, *forced, *table, rank, rs.flags, R, S, bool(timed))
            if rings is None:
                ms = _ops.backend().rank_frames(*args)
            else:
                ms = getattr(_ops.backend(), rings.op)(*args, *rings.op_args(R, S))
            if timed:
                self.last_step_ms = ms.numpy()
            if rings is not None:
                rings.check()
            rs.check_flags("rank_rows_kernel flagged a target outside the vocabulary (flags %d)",
                           "the logit of a target word is NaN: its rank is undefined")
            out = rank.cpu().numpy()
        return (out,) + rs.after(S)

    def sentences(self, sequences, start, levels, max_rows, limit, spec=None, patch=None, extra_bytes=None):
        """rank_sequences, and with ``spec`` (a checked CacheSpec) jlm_amd.cache.rank_cached: every chunk with rings of its own; with
        ``patch`` (word [S, R] -> a jlm_amd.ngram_mix.NgramPatch) jlm_amd.ngram_mix.rank_ngram: every chunk with its histories;
        ``extra_bytes`` (n_steps -> bytes): what the patch's own buffers add to a row of a call (jlm_amd.memory.rank_memory)"""
        L = levels.n_levels if levels is not None else 0
        more = extra_bytes or (lambda n: 0)

        def run(ch, word, target, lens):
            rings = MixRings(self.m, spec, len(lens), ch["n_steps"]) if spec else patch(word) if patch else None
            rk = self.run(word, target, ch["n_live"], levels=levels, rings=rings)[0]
            return [_columns(levels, rk[:n, r, :], target[:n, r]) for r, n in enumerate(lens)]
        return sentence_loop(self.m, sequences, start, "rank", max_rows, limit, lambda n: self.row_bytes(n, L, spec.size if spec else 0, ngram=patch is not None and extra_bytes is None) + more(n),
                             lambda n: np.full((n, L + 1), -1, dtype=np.int32), run)

    def streams(self, x, y, h, c, levels, rings=None):
        """a stream call of the checked x, y [B, n] -> (ranks [B, n, columns] in the public columns, h, c)"""
        B, n = x.shape
        rk, h2, c2 = self.run(x.T, y.T, [B] * n, h=h, c=c, levels=levels, rings=rings)
        flat = _columns(levels, rk.reshape(n * B, -1), np.ascontiguousarray(y.T).reshape(-1))
        return np.ascontiguousarray(flat.reshape(n, B, -1).transpose(1, 0, 2)), h2, c2


def _columns(levels, dev_rank, target):
    return dev_rank if levels is None else levels.to_columns(dev_rank, target)


def rank_sequences(ranker, sequences, start, levels=None, max_rows=None):
    """LSTM_Model.rank: see there."""
    return ranker.sentences(sequences, start, levels, max_rows, (MAX_ROWS, GENERATE_BUDGET_BYTES))


def rank_streams(ranker, inputs, targets, h=None, c=None, levels=None):
    """LSTM_Model.rank_streams: see there."""
    x, y, B, n = check_streams(ranker.m, inputs, targets, h, c)
    if B == 0 or n == 0:
        L = levels.n_levels if levels is not None else 0
        return np.full((B, n, L + 1), -1, dtype=np.int32), h, c
    return ranker.streams(x, y, h, c, levels)


# ---------------------------------------------------------------------------------------------------------------- metrics (numpy)
def _stack(ranks):
    """one [N, columns] array of a rank array, or of a list of them (LSTM_Model.rank's result; [B, n, columns] of rank_streams)"""
    if isinstance(ranks, np.ndarray):
        a = ranks
    else:
        parts = [np.asarray(r) for r in ranks]
        a = np.concatenate([p.reshape(-1, p.shape[-1]) for p in parts]) if parts else np.zeros((0, 1), dtype=np.int32)
    return a.reshape(-1, a.shape[-1]).astype(np.int64)


def reading_lengths(index):
    """[V] int64: the number of kana of every word's reading in a :class:`jlm_amd.readings.ReadingIndex`, 0 for a word without one"""
    out = np.zeros(index.V, dtype=np.int64)
    out[index.ids] = [len(r) for r in index.readings]
    return out


def topk_accuracy(ranks, ks):
    """-> {k: the share of tokens whose target is among the k most probable words} (column A < k)"""
    a = _stack(ranks)[:, 0]
    return {int(k): (float(np.mean((a >= 0) & (a < k))) if len(a) else float("nan")) for k in ks}


def mrr(ranks):
    """the mean reciprocal rank 1 / (rank + 1) of column A"""
    a = _stack(ranks)[:, 0]
    a = a[a >= 0]
    return float(np.mean(1.0 / (a + 1.0))) if len(a) else float("nan")


def keystrokes(ranks, reading_lengths, list_size):
    """Keystroke savings of a candidate list of ``list_size`` words.  ``ranks``: arrays with the prefix columns (``readings=True``);
    ``reading_lengths``: the number of kana of each token's reading, in the same order (0: no reading).  A token of l >= 1 kana costs
    typed = min{ j <= min(l, max_prefix) : rank_j < list_size } kana -- the first moment its word is in the list -- and l when there
    is no such j; savings = 1 - sum typed / sum l.  Tokens without a reading are excluded and counted.  The keystroke that SELECTS
    the word from the list is not counted, on either side: with it, a word offered only once it is typed in full saves nothing and
    costs one key more.  -> dict(savings, typed, kana, tokens, excluded)"""
    a = _stack(ranks)
    if a.shape[1] < 3:
        raise ValueError("keystrokes needs the prefix levels (rank(..., readings=True))")
    ell = np.asarray(reading_lengths, dtype=np.int64).reshape(-1)
    if len(ell) != len(a):
        raise ValueError("one reading length per token (%d tokens, %d lengths)" % (len(a), len(ell)))
    if list_size < 1:
        raise ValueError("list_size must be >= 1")
    max_prefix = a.shape[1] - 3
    pre = a[:, 1:max_prefix + 2]                                   # prefix levels 0 .. max_prefix
    j = np.arange(max_prefix + 1)[None, :]
    hit = (pre >= 0) & (pre < list_size) & (j <= ell[:, None])
    first = np.where(hit.any(axis=1), hit.argmax(axis=1), ell)
    keep = ell >= 1
    typed, kana = int(first[keep].sum()), int(ell[keep].sum())
    return dict(savings=(1.0 - typed / kana) if kana else float("nan"), typed=typed, kana=kana, tokens=int(keep.sum()),
                excluded=int((~keep).sum()))


def homophone_position(ranks):
    """the position of the target among its homophones (column X, the last): -> dict(mean, first = the share at position 0, tokens)
    over the tokens that have a reading"""
    a = _stack(ranks)
    if a.shape[1] < 3:
        raise ValueError("homophone_position needs level X (rank(..., readings=True))")
    x = a[:, -1]
    x = x[x >= 0]
    if not len(x):
        return dict(mean=float("nan"), first=float("nan"), tokens=0)
    return dict(mean=float(x.mean()), first=float(np.mean(x == 0)), tokens=int(len(x)))
