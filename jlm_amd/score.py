"""Teacher-forced scoring on the device: the per-word -log p of many word sequences at once.

The reference measures a model by its test perplexity (train/train.py:101-102 over train/model.py:262-297) and scores a sentence
with ``LSTM_Model.evaluate`` (decoder/model.py:200-206), one ``predict()`` -- one materialised softmax -- per word.  Here a call is
ONE op (``torch.ops.jlm.score_frames``, csrc/jlm_decode.hip ``jlm_score_frames``): per step the LSTM step of the live rows, the T
projection, the full-vocabulary normaliser the decoders use, and ``score_fold_kernel`` (csrc/jlm_score.hip), which folds the
normaliser's slices and takes the target word's logit.  Nothing comes back to the host between steps.

Host logic of this module (row plan, stream layout, id checks) is plain numpy; :class:`Scorer` owns the device buffers of a call.
``LSTM_Model.score`` / ``score_streams`` (jlm_amd/model.py) are the public entry points, over :func:`score_sequences` and
:func:`score_streams` here; ``python -m jlm_amd.perplexity`` is the command-line front end.  :func:`sentence_loop` is the sentence mode
of every teacher-forced call: score and rank (jlm_amd/rank.py) and their cached forms (jlm_amd/cache.py).
"""
import numpy as np

from . import ops as _ops
from .rowsets import RowSets, check_ids, check_streams, clamp_rows, forced_rows

# rows per call: the gate GEMM is most efficient at large row counts (37-40 % of the MFMA peak at 20 480 rows, 28 % at 2 560:
# BENCH_r06); a call's buffers are bounded by SCORE_BUDGET_BYTES besides
MAX_ROWS = 20480
SCORE_BUDGET_BYTES = 2 << 30


def plan_rows(lengths, max_rows):
    """The row plan of a sentence-mode call.  Sequences are sorted by length, longest first (stable), so that the rows live at step t
    -- those with a word left to score -- are a prefix; empty sequences take no row.  -> list of chunks of at most ``max_rows`` rows:
    dict(idx = the sequence of each row, lens = their lengths, n_steps = the longest, n_live [n_steps] = live rows per step)."""
    if max_rows < 1:
        raise ValueError("max_rows must be >= 1")
    lens = np.asarray(lengths, dtype=np.int64)
    order = np.argsort(-lens, kind="stable")
    order = order[lens[order] > 0]
    chunks = []
    for i in range(0, len(order), max_rows):
        idx = order[i:i + max_rows]
        L = lens[idx]
        n_steps = int(L[0])
        n_live = (L[None, :] > np.arange(n_steps)[:, None]).sum(axis=1).astype(np.int32)
        chunks.append(dict(idx=idx, lens=L, n_steps=n_steps, n_live=n_live))
    return chunks


def sentence_arrays(seqs, start, n_steps):
    """word / target [n_steps, R] int32 of the rows ``seqs`` (longest first): step 0 consumes ``start``, step t consumes s[t - 1] and is
    scored on s[t]; positions past a row's end hold 0 (never read: the row is not live there)."""
    R = len(seqs)
    word = np.zeros((n_steps, R), dtype=np.int32)
    target = np.zeros((n_steps, R), dtype=np.int32)
    word[0, :] = start
    for r, s in enumerate(seqs):
        L = len(s)
        target[:L, r] = s
        word[1:L, r] = s[:L - 1]
    return word, target


def stream_layout(data, batch_size, num_steps):
    """The reference's corpus_iterator (train/utils.py:17-31) as two arrays: the id stream cut into ``batch_size`` rows of
    batch_len = len // batch_size ids (the tail dropped), of which the first epoch_size * num_steps steps are read,
    epoch_size = (batch_len - 1) // num_steps.  -> (inputs, targets) [batch_size, epoch_size * num_steps] int32, targets shifted
    by one; chunk i of the iterator is columns [i * num_steps, (i + 1) * num_steps)."""
    raw = np.asarray(data, dtype=np.int32)
    batch_len = len(raw) // batch_size
    rows = raw[:batch_size * batch_len].reshape(batch_size, batch_len)
    epoch_size = (batch_len - 1) // num_steps
    if epoch_size <= 0:
        raise ValueError("epoch_size == 0, decrease batch_size or num_steps")
    n = epoch_size * num_steps
    return np.ascontiguousarray(rows[:, :n]), np.ascontiguousarray(rows[:, 1:n + 1])


class Scorer:
    """The device side of a scoring call over a :class:`jlm_amd.model.DeviceModel`."""

    def __init__(self, dev_model):
        self.m = dev_model
        self.torch = dev_model.torch
        self.last_step_ms = None          # [n_steps, 4] of the last timed call: LSTM step, T projection, normaliser, fold

    def row_bytes(self, n_steps, per_token=True, cache_size=0, n_theta=1):
        """bytes of a call's buffers per row; cache_size = N > 0: with the rings of a cached call, (N + n) state rows and words, and
        its lpc (jlm_amd/cache.py)"""
        m = self.m
        n_parts = 0 if m.self_norm else max(m.n_vocab_tiles, 1)
        plain = (4 * m.H + m.ldt + (m.ld_tm or 0)) * 4 + n_parts * 8 + 16 + n_steps * (8 + (8 if per_token else 0))
        if not cache_size:
            return plain
        return plain + (cache_size + n_steps) * (m.H * 4 + 4) + 4 * n_theta * n_steps + 8

    def run(self, word, target, n_live, h=None, c=None, per_token=True, timed=False, rings=None):
        """One call: word / target [n_steps, R] int32 (host), n_live [n_steps] (host; non-increasing, rows live as a prefix).  h, c:
        the state to continue ([R, H] device tensors in the model's state-row format, as returned here), None = the zero state.
        rings: a :class:`jlm_amd.cache.Rings` made for this call's (R, n_steps) -- the op is then ``score_cache_frames``, the same
        launches with the cache pass behind them, and the rings hold the call's states, words and lpc afterwards -- or a
        :class:`jlm_amd.memory.MemoryRings`, whose ``op`` names ``score_memory_frames``: the same launches with the memory pass behind.
        -> (nll_seq [R] f64, nll_tok [n_steps, R] f64 or None, h, c) -- numpy results, the state after the last step on the device.
        The returned h, c are the row set the LAST step wrote: they hold the final state of the rows live at that step.  A row that
        stopped being live earlier is UNDEFINED there (its final state is in the other set when its length and n_steps differ in
        parity, and its slot here is unwritten or one step old): ragged callers do not carry a state."""
        torch, m = self.torch, self.m
        dev, f64 = m.device, torch.float64
        with m._ctx():
            R = np.shape(target)[1]
            rs = RowSets(m, R)
            part, n_parts = None, 0
            if not m.self_norm:
                n_parts = max(m.n_vocab_tiles, 1)
                part = torch.empty((n_parts, R, 2), device=dev, dtype=torch.float32)
            Tm = None
            if part is not None and getattr(m, "ld_tm", 0):
                Tm = torch.zeros(((R + 31) // 32 * 32, m.ld_tm), device=dev, dtype=torch.float32)     # whole 32-row blocks (jlm_hip.h)
            S, R, forced = forced_rows(m, rs, word, target, n_live, h, c, "score")
            nll_seq = torch.zeros(R, device=dev, dtype=f64)
            nll_tok = torch.zeros((S, R), device=dev, dtype=f64) if per_token else None
            args = (m.decode_model(), *rs.state(), Tm, int(m.ld_tm or 0), part, n_parts, *forced, nll_seq, nll_tok, rs.flags, R, S, bool(timed))
            if rings is None:
                ms = _ops.backend().score_frames(*args)
            else:
                ms = getattr(_ops.backend(), getattr(rings, "op", "score_cache_frames"))(*args, *rings.op_args(R, S))
            if timed:
                self.last_step_ms = ms.numpy()
            rs.check_flags("score_fold_kernel flagged a target outside the model's segments (flags %d)",
                           "a log-normaliser is not finite: this model's logits left the range the fixed-reference normaliser covers "
                           "(DeviceModel.mixed_calib); set JLM_MX_FIXREF=0")
            seq = nll_seq.cpu().numpy()
            tok = nll_tok.cpu().numpy() if per_token else None
        return (seq, tok) + rs.after(S)


def sentence_loop(m, sequences, start, what, max_rows, limit, row_bytes, empty, run):
    """The sentence mode of score, rank and their cached forms (``what``: "score" / "rank", the label of the id errors).  The
    sequences and ``start`` are checked, sorted and cut into chunks of at most ``max_rows`` rows -- None: ``limit`` = (rows, bytes) a
    call, with ``row_bytes(longest)`` bytes a row -- and each chunk runs as ``run(chunk, word, target, lens)`` (:func:`plan_rows`,
    :func:`sentence_arrays`; lens: the rows' lengths as a list), which returns the result of every row of the chunk.  -> per sequence,
    in input order, its row's result; ``empty(n)`` for a sequence that took no row."""
    seqs = [np.asarray(s, dtype=np.int64).ravel() for s in sequences]
    for s in seqs:
        check_ids(s, m.V, what)
    check_ids([start], m.V, what + " (start)")
    lens = [len(s) for s in seqs]
    if max_rows is None:
        max_rows = clamp_rows(*limit, row_bytes(max(lens, default=0)), m.H)
    out = [empty(n) for n in lens]
    for ch in plan_rows(lens, max_rows):
        word, target = sentence_arrays([seqs[i] for i in ch["idx"]], start, ch["n_steps"])
        for i, res in zip(ch["idx"], run(ch, word, target, ch["lens"].tolist())):
            out[i] = res
    return out


def score_sequences(scorer, sequences, start, per_token=True, max_rows=None):
    """LSTM_Model.score: see there."""
    def run(ch, word, target, lens):
        seq, tok, _h, _c = scorer.run(word, target, ch["n_live"], per_token=per_token)
        return [tok[:n, r].copy() for r, n in enumerate(lens)] if per_token else seq
    out = sentence_loop(scorer.m, sequences, start, "score", max_rows, (MAX_ROWS, SCORE_BUDGET_BYTES), lambda n: scorer.row_bytes(n, per_token),
                        (lambda n: np.zeros(n, dtype=np.float64)) if per_token else (lambda n: 0.0), run)
    return out if per_token else np.asarray(out, dtype=np.float64)


def score_streams(scorer, inputs, targets, h=None, c=None):
    """LSTM_Model.score_streams: see there."""
    x, y, B, n = check_streams(scorer.m, inputs, targets, h, c)
    if B == 0 or n == 0:
        return np.zeros((B, n), dtype=np.float64), h, c
    _seq, tok, h2, c2 = scorer.run(x.T, y.T, [B] * n, h=h, c=c, per_token=True)
    return np.ascontiguousarray(tok.T), h2, c2
