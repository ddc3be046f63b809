"""Ranking, prediction and completion under the back-off n-gram mixture: the host side of
``LSTM_Model.rank_streams_ngram`` / ``rank_ngram`` and of the ``ngram=`` keyword of ``predict_top`` / ``predict_reading`` / ``complete``
/ ``complete_reading``.

``Decoder.decode(ngram=)`` (section 24) looks single (history, word) pairs up; here every step's full-vocabulary logits are patched on
the device into the logits of the mixture (1 - lam) p_lm + lam q(. | history) -- ``jlm_amd.ngram.mixed_logits`` is the float64
statement, csrc/jlm_ngram_mix.hip the kernel -- and the ranking and selection kernels run unchanged on the patched rows.  A teacher-
forced call knows every history and uploads them; a beam search carries the last two words of every hypothesis on the device.

What the kernels report is -log of the ROW-NORMALISED mixture p_mix(w) / ((1 - lam) + lam Z_h), Z_h = sum_w exp q(w | h): p_mix itself
for a table that sums to one (``jlm_amd.ngram.estimate``'s do), and off by a constant per row -- which changes no rank and no order --
for a file whose out-of-vocabulary n-grams were dropped.  On self-normalised models they report -y', and -log1p(-lam) is added here.
"""
import numpy as np

from . import _lib
from .ngram import check_mix_rows, successor_tensors
from .rowsets import check_streams, is_int


def _flag_error(fl):
    if fl & 2:
        return _lib.JlmHipError("ngram_mix_rows_kernel flagged a row whose log-normaliser is not finite")
    return _lib.JlmHipError("ngram_mix_rows_kernel flagged a history word outside the vocabulary (flags %d)" % fl)


def table_args(m, ngram):
    """the ops' run of table arguments: the 11 tensors, [n_bi, n_tri, n_ctx, log2cap, max_probe], order, lam"""
    from .ngram import SUCCESSOR_TENSORS
    tens, arr = successor_tensors(ngram.table, m.V, m.device)
    sizes = [int(arr["bi_w"].size), int(arr["tri_w"].size), int(arr["n_ctx"]), int(arr["log2cap"]), int(arr["max_probe"])]
    return [tens[k] for k in SUCCESSOR_TENSORS], sizes, int(ngram.table.order), float(ngram.lam)


def forced_hist(word, first=None):
    """hist [S, R, 2] int32 of a teacher-forced call from the words its steps consume, word [S, R]: step t ranks under the history
    (word[t - 1], word[t]); ``first`` [R]: the word before word[0] (None: none, -1)"""
    word = np.asarray(word, dtype=np.int32)
    hist = np.empty(word.shape + (2,), dtype=np.int32)
    hist[..., 1] = word
    hist[1:, :, 0] = word[:-1]
    hist[0, :, 0] = -1 if first is None else first
    return hist


class NgramPatch:
    """What ``Ranker.run`` passes ``rank_ngram_frames`` behind ``rank_frames``' arguments (jlm_ngram_mix_plan): the table, the uploaded
    histories hist [S, R, 2] and, ``top`` > 0, the lists top_ids / top_nll [S, R, top] of every step."""
    op = "rank_ngram_frames"

    def __init__(self, m, ngram, hist, top=0):
        torch, dev = m.torch, m.device
        self.m, self.ngram, self.top = m, ngram, int(top)
        S, R = hist.shape[:2]
        with m._ctx():
            self.table = table_args(m, ngram)
            self.hist = torch.from_numpy(np.ascontiguousarray(hist, dtype=np.int32)).to(dev)
            self.top_ids = torch.full((S, R, self.top), -1, device=dev, dtype=torch.int32) if self.top else None
            self.top_nll = torch.full((S, R, self.top), float("nan"), device=dev, dtype=torch.float64) if self.top else None
            self.flags = torch.zeros(1, device=dev, dtype=torch.int32)

    def op_args(self, R, S):
        return (*self.table, self.hist, self.top, self.top_ids, self.top_nll, self.flags)

    def check(self):
        fl = int(self.flags.cpu()[0])
        if fl:
            raise _flag_error(fl)

    def lists(self):
        """(top_ids [S, R, top] int64, top_logp [S, R, top] float64) -- after the op"""
        ids = self.top_ids.cpu().numpy().astype(np.int64)
        logp = -self.top_nll.cpu().numpy()
        if self.m.self_norm:
            logp = logp + np.log1p(-float(np.float32(self.ngram.lam)))
        return ids, logp


class NgramRanks:
    """What ``rank_streams_ngram`` returns.  ``ranks`` [B, n, columns] int32: rank_streams' array under the mixture; ``top_ids``
    [B, n, top] int64 / ``top_logp`` [B, n, top] float64 (most probable first) when ``top`` > 0, else None; ``h``, ``c``, ``tail``:
    what the next call of the stream carries."""

    def __init__(self, ranks, h, c, tail, top_ids, top_logp):
        self.ranks, self.h, self.c, self.tail, self.top_ids, self.top_logp = ranks, h, c, tail, top_ids, top_logp


def check_tail(tail, B, V):
    """``tail``: None (no word before the stream) or int [B, 2], the last two words before inputs[:, 0], -1 meaning none"""
    if tail is None:
        return np.full((B, 2), -1, dtype=np.int32)
    t = np.asarray(tail)
    if t.shape != (B, 2) or t.dtype.kind not in "iu":
        raise ValueError("tail must be an integer array [%d, 2] (got %s)" % (B, t.shape))
    if t.size and (t.min() < -1 or t.max() >= V):
        raise ValueError("tail: a word id outside [-1, %d)" % V)
    return t.astype(np.int32)


def check_top(top, V):
    if not is_int(top) or not 0 <= top <= min(64, V):
        raise ValueError("top must be an integer in [0, %d] (got %r)" % (min(64, V), top))
    return int(top)


def rank_streams_ngram(ranker, inputs, targets, ngram, h=None, c=None, tail=None, levels=None, top=0):
    """LSTM_Model.rank_streams_ngram: see there."""
    m = ranker.m
    check_mix_rows(ngram, m.V)
    top = check_top(top, m.V)
    x, y, B, n = check_streams(m, inputs, targets, h, c, "rank")
    tail = check_tail(tail, B, m.V)
    L = levels.n_levels if levels is not None else 0
    if B == 0 or n == 0:
        return NgramRanks(np.full((B, n, L + 1), -1, dtype=np.int32), h, c, tail, np.zeros((B, n, top), dtype=np.int64) if top else None,
                          np.zeros((B, n, top)) if top else None)
    patch = NgramPatch(m, ngram, forced_hist(x.T, tail[:, 1]), top)
    ranks, h2, c2 = ranker.streams(x, y, h, c, levels, patch)
    ids = logp = None
    if top:
        ids, logp = patch.lists()
        ids, logp = np.ascontiguousarray(ids.transpose(1, 0, 2)), np.ascontiguousarray(logp.transpose(1, 0, 2))
    after = np.concatenate([tail, x.astype(np.int32)], axis=1)[:, -2:]
    return NgramRanks(ranks, h2, c2, np.ascontiguousarray(after), ids, logp)


def rank_ngram(ranker, sequences, start, ngram, levels=None, max_rows=None):
    """LSTM_Model.rank_ngram: see there."""
    from .generate import GENERATE_BUDGET_BYTES, MAX_ROWS
    m = ranker.m
    check_mix_rows(ngram, m.V)
    return ranker.sentences(sequences, start, levels, max_rows, (MAX_ROWS, GENERATE_BUDGET_BYTES),
                            patch=lambda word: NgramPatch(m, ngram, forced_hist(word)))


class BeamHist:
    """What ``Completer.run`` passes ``complete_frames_ngram`` behind ``complete_frames_masked``' arguments (jlm_complete_ngram_plan):
    the table and the two history buffers [R, 2], the first holding the last two words of every prompt."""

    def __init__(self, m, ngram, prompts, R):
        torch, dev = m.torch, m.device
        h0 = np.full((R, 2), -1, dtype=np.int32)
        for p, words in enumerate(prompts):
            last = np.asarray(words, dtype=np.int32)[-2:]
            h0[p, 2 - len(last):] = last
        self.ngram = ngram
        self.table = table_args(m, ngram)
        self.hist = [torch.from_numpy(h0).to(dev), torch.full((R, 2), -1, device=dev, dtype=torch.int32)]
        self.flags = torch.zeros(1, device=dev, dtype=torch.int32)

    def op_args(self):
        return (*self.table, self.hist[0], self.hist[1], self.flags)

    def check(self):
        fl = int(self.flags.cpu()[0])
        if fl:
            raise _flag_error(fl)
