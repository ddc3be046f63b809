"""A continuous cache for teacher-forced scoring: adaptation to the text already written, with no training (Grave, Joulin, Usunier,
"Improving neural language models with a continuous cache", ICLR 2017).

The model is static; the cache keeps the last N hidden states of a row together with the word that followed each, gives the next
word the mass softmax(theta h_t . h_i) puts on the earlier positions that were followed by that word, and interpolates that mass with
the model's probability.  Definition (include/jlm_hip.h): position j is the step that consumes word[j], leaves
h_j and is scored on w_j = target[j]; positions are numbered over the whole life of a stream; before position q the cache holds
(h_i, w_i) for max(q - N, first) <= i < q, n_q of them;

    s_i       = theta (h_q . h_i)
    lpc_q     = log sum_{i : w_i = w_q} exp(s_i) - log sum_i exp(s_i)          (-inf when no i matches)
    p_q       = (1 - lam) exp(-nll_q) + lam exp(lpc_q)  when n_q > 0;  exp(-nll_q)  when n_q = 0
    nll_mix_q = -log p_q                                                        (float64, here, via logaddexp)

A call is ONE op (``torch.ops.jlm.score_cache_frames``, csrc/jlm_decode.hip ``jlm_score_cache_frames``): ``score_frames``' launches,
the written state rows copied into a ring after every step, and ``cache_rows_kernel`` (csrc/jlm_cache.hip) once behind the last step.
lpc does not depend on lam, so lam is swept on the host from one device pass (:func:`tune`).

``LSTM_Model.score_cached`` / ``score_streams_cached`` (jlm_amd/model.py) are the public entry points, ``python -m jlm_amd.perplexity
--cache`` the command-line front end.  :class:`Ring` is the ring of a cached call; :class:`Rings` (scoring) and :class:`MixRings`
(ranking) add their ops' own buffers.

Ranking and prediction need the cache's mass on EVERY word of the window, not the target's alone:

    c_q(w) = sum_{i in window, w_i = w} exp(s_i) / sum_{i in window} exp(s_i)
    p_q(w) = (1 - lam) p_lm(w) + lam c_q(w)  when n_q > 0 and lam > 0;  p_lm(w) otherwise;  p_lm(w) = exp(y[w] - L), L = lse(y) (self_norm: 0)
    y'[w]  = logaddexp(y[w], L + log(lam / (1 - lam)) + log c_q(w))  on the words of the window,  y[w] elsewhere

-- ordering by y' is ordering by p_q, and lse(y') = L - log(1 - lam).  :func:`cache_distribution` and :func:`mixed_logits` state it
in float64; on the device ``torch.ops.jlm.rank_cache_frames`` patches every step's logits (csrc/jlm_cache_mix.hip) before
``rank_rows_kernel`` / ``topk_rows_kernel`` read them: ``LSTM_Model.rank_streams_cached`` / ``rank_cached`` / ``predict_next_cached``.
"""
import numpy as np

from . import _lib
from . import ops as _ops
from .complete import check_allowed
from .generate import GENERATE_BUDGET_BYTES
from .readings import ReadingIndex
from .rowsets import RowSets, check_streams, is_int, t_is_state
from .score import MAX_ROWS, SCORE_BUDGET_BYTES, sentence_loop

MAX_THETAS = 16                     # JLM_CACHE_MAX_THETAS
MAX_SIZE = 1 << 24


class CacheSpec:
    """What a cached call is asked for: ``size`` = N >= 1 entries, ``theta`` >= 0 -- one value or a sequence of 1 .. 16 for tuning
    (one device pass serves them all) -- and 0 <= ``lam`` < 1.  ValueError for anything else, here, before anything runs."""

    def __init__(self, size, theta=0.3, lam=0.1):
        if not is_int(size) or not 1 <= size <= MAX_SIZE:
            raise ValueError("cache size must be an integer in [1, %d] (got %r)" % (MAX_SIZE, size))
        raw = list(theta) if isinstance(theta, (list, tuple, np.ndarray)) else [theta]
        if not 1 <= len(raw) <= MAX_THETAS:
            raise ValueError("1 .. %d values of theta a call (got %d)" % (MAX_THETAS, len(raw)))
        th = []
        for x in raw:
            if isinstance(x, bool) or not isinstance(x, (int, float, np.integer, np.floating)) or not 0 <= x < 3.0e38:
                raise ValueError("theta must be a finite number >= 0 (got %r)" % (x,))
            th.append(float(x))
        check_lam(lam)
        self.size, self.thetas, self.lam = int(size), tuple(th), float(lam)

    @property
    def theta(self):
        return self.thetas[0]


def check_lam(lam):
    if isinstance(lam, bool) or not isinstance(lam, (int, float, np.integer, np.floating)) or not 0 <= lam < 1:
        raise ValueError("lam must be a number in [0, 1) (got %r)" % (lam,))
    return float(lam)


def _check_spec(cache):
    if not isinstance(cache, CacheSpec):
        raise ValueError("cache must be a CacheSpec (got %r)" % (cache,))
    return cache


# ---------------------------------------------------------------------------------------------------------------- the definition (float64)
def cache_log_probs(h, words, size, thetas, carried=0):
    """The definition for ONE row, in float64.  ``h`` [n, H]: the states h_i in real units, ``words`` [n]: w_i, the first ``carried``
    of them entries that were there before the first query (queries: positions carried .. n - 1); the row's oldest existing position
    is 0.  -> (lpc [n_theta, n - carried] float64 with -inf where nothing matches or the cache is empty, n_entries [n - carried])."""
    h = np.asarray(h, dtype=np.float64)
    w = np.asarray(words)
    n = len(w)
    th = np.atleast_1d(np.asarray(thetas, dtype=np.float64))
    lpc = np.full((len(th), n - carried), -np.inf)
    cnt = np.zeros(n - carried, dtype=np.int64)
    for q in range(carried, n):
        lo = max(q - size, 0)
        cnt[q - carried] = q - lo
        if q == lo:
            continue
        dot = h[lo:q] @ h[q]
        same = w[lo:q] == w[q]
        if not same.any():
            continue
        for t, theta in enumerate(th):
            s = theta * dot
            top = s.max()
            e = np.exp(s - top)
            lpc[t, q - carried] = np.log(e[same].sum()) - np.log(e.sum())
    return lpc, cnt


def mix_nll(nll_lm, lpc, n_entries, lam):
    """nll_mix of the definition, float64: -logaddexp(log(1 - lam) - nll_lm, log(lam) + lpc) where n_entries > 0, nll_lm elsewhere;
    lam = 0 returns nll_lm's bits."""
    lam = check_lam(lam)
    nll = np.asarray(nll_lm, dtype=np.float64)
    if lam == 0.0:
        return nll.copy()
    with np.errstate(invalid="ignore"):
        mixed = -np.logaddexp(np.log1p(-lam) - nll, np.log(lam) + np.asarray(lpc, dtype=np.float64))
    return np.where(np.asarray(n_entries) > 0, mixed, nll)


def cache_distribution(h, words, size, theta, V, carried=0):
    """The cache distribution over EVERY word, for ONE row, in float64 (include/jlm_hip.h jlm_cache_query / jlm_cache_mix_rows,
    DESIGN.md section 20).  ``h`` [n, H], ``words`` [n], ``carried`` as :func:`cache_log_probs` takes them; one ``theta``.
    -> (c [n - carried, V] float64: c_q(w) = sum_{i in window, w_i = w} exp(s_i) / sum_{i in window} exp(s_i), a row of zeros where the
    window is empty; n_entries [n - carried]).  log c_q(w_q) is lpc_q of :func:`cache_log_probs`."""
    h = np.asarray(h, dtype=np.float64)
    w = np.asarray(words, dtype=np.int64)
    n = len(w)
    if n and (w.min() < 0 or w.max() >= V):
        raise ValueError("a cached word is outside [0, %d)" % V)
    c = np.zeros((n - carried, V))
    cnt = np.zeros(n - carried, dtype=np.int64)
    for q in range(carried, n):
        lo = max(q - size, 0)
        cnt[q - carried] = q - lo
        if q == lo:
            continue
        s = float(theta) * (h[lo:q] @ h[q])
        e = np.exp(s - s.max())
        np.add.at(c[q - carried], w[lo:q], e)
        c[q - carried] /= e.sum()
    return c, cnt


def mixed_logits(y, c, lam, self_norm=False):
    """y' of the definition, float64: rows ``y`` [..., V] of logits and ``c`` [..., V] of :func:`cache_distribution` ->
    logaddexp(y, L + log(lam / (1 - lam)) + log c) where c > 0 and y where c = 0, L = lse(y) over the row (``self_norm``: 0).  Ordering
    a row by y' is ordering it by p = (1 - lam) p_lm + lam c, and lse(y') = L - log(1 - lam).  lam = 0 and a row whose c is all zero (an
    empty window) return y's bits."""
    lam = check_lam(lam)
    y = np.asarray(y, dtype=np.float64)
    c = np.asarray(c, dtype=np.float64)
    if y.shape != c.shape:
        raise ValueError("y and c must have the same shape (got %s, %s)" % (y.shape, c.shape))
    if lam == 0.0:
        return y.copy()
    if self_norm:
        L = np.zeros(y.shape[:-1] + (1,))
    else:
        top = y.max(axis=-1, keepdims=True)
        L = top + np.log(np.exp(y - top).sum(axis=-1, keepdims=True))
    with np.errstate(divide="ignore", invalid="ignore"):          # (log 0 = -inf where c = 0: those entries are y's)
        term = L + (np.log(lam) - np.log1p(-lam)) + np.log(c)
        return np.where(c > 0, np.logaddexp(y, term), y)


# ---------------------------------------------------------------------------------------------------------------- device side
def decode_rows(m, raw):
    """state rows [..., H] of the device's format as float32 on the host: split rows decoded as ContextState.numpy does (hi + lo, the
    scale divided out)"""
    raw = raw.detach().cpu().contiguous().numpy()
    if m.split_lstm:
        sp = raw.view(np.float16).reshape(raw.shape[:-1] + (m.H // 8, 2, 8)).astype(np.float64)
        return ((sp[..., 0, :] + sp[..., 1, :]).reshape(raw.shape[:-1] + (m.H,)) / float(m.h_scale)).astype(np.float32)
    return raw.astype(np.float32)


class CacheState:
    """The last ``count`` <= N (h, word) of ``n_rows`` streams on the device of a :class:`jlm_amd.model.DeviceModel`; nothing in it is
    written after it is made.  ``hist`` [count, n_rows, H] in the model's state-row format (4 bytes a value), ``words`` [count, n_rows]
    int32, entry k being logical position ``pos - count + k`` of its stream; ``pos``: the position of the stream's next step."""

    def __init__(self, m, hist, words, pos):
        self.m, self.hist, self.words, self.pos = m, hist, words, int(pos)
        self.count, self.n_rows = int(words.shape[0]), int(words.shape[1])

    @property
    def positions(self):
        return np.arange(self.pos - self.count, self.pos, dtype=np.int64)

    def numpy(self):
        """(h [n_rows, count, H] float32 with split rows decoded, words [n_rows, count] int64, positions [count] int64)"""
        h = decode_rows(self.m, self.hist).transpose(1, 0, 2)
        return np.ascontiguousarray(h), np.ascontiguousarray(self.words.detach().cpu().numpy().T.astype(np.int64)), self.positions


class Ring:
    """The ring of one cached call of R rows and S steps: cap = N + S slots of (h, word), the carried entries at the local positions
    0 .. carried - 1 and the call's steps at carried .. carried + S - 1 -- a call numbers positions from its oldest carried entry, so
    ``first`` is 0 and no slot wraps; :class:`CacheState` keeps the stream's own numbering.  A subclass gives the slots' memory with
    the carried entries at its front (``_slots``) and adds its op's own buffers; it constructs inside the model's context."""

    def __init__(self, m, spec, R, S, state=None):
        torch, dev = m.torch, m.device
        self.m, self.spec, self.R, self.S = m, spec, R, S
        self.carried = min(state.count, spec.size) if state is not None else 0
        self.cap = spec.size + S
        k = self.carried
        self.hist = self._slots((self.cap, R, m.H), torch.float32, state.hist[state.count - k:].view(torch.float32) if k else None)
        self.words = self._slots((self.cap, R), torch.int32, state.words[state.count - k:] if k else None)
        self.first = torch.zeros(R, device=dev, dtype=torch.int32)
        self.flags = torch.zeros(1, device=dev, dtype=torch.int32)

    def ring_args(self, R, S):
        """the ops' argument run hist, words, cap, pos, first"""
        if (R, S) != (self.R, self.S):
            raise ValueError("these rings were made for %d rows and %d steps (got %d, %d)" % (self.R, self.S, R, S))
        return self.hist, self.words, self.cap, self.carried, self.first

    def n_entries(self):
        """[S]: the entries of a live row's window at each step"""
        return np.minimum(self.carried + np.arange(self.S, dtype=np.int64), self.spec.size)

    def state_after(self, pos):
        """the CacheState after the call's S steps (every row live to the end), the stream's next position being ``pos``"""
        end = self.carried + self.S
        cnt = min(end, self.spec.size)
        # (views: the rings are not written after the call, and a copy of N state rows a call costs as much as the cache pass)
        return CacheState(self.m, self.hist[end - cnt:end], self.words[end - cnt:end], pos)


class Rings(Ring):
    """The rings of one cached scoring call (jlm_cache_plan): :class:`Ring` in uninitialised memory -- every slot is written before it
    is read -- with ``lens`` [R], the steps each row is live, and lpc [n_theta, S, R]."""

    def __init__(self, m, spec, R, S, lens, state=None):
        torch, dev = m.torch, m.device
        with m._ctx():
            super().__init__(m, spec, R, S, state)
            self.len = torch.from_numpy(np.ascontiguousarray(lens, dtype=np.int32)).to(dev)
            self.lpc = torch.full((len(spec.thetas), S, R), float("-inf"), device=dev, dtype=torch.float32)

    def _slots(self, shape, dtype, front):
        t = self.m.torch.empty(shape, device=self.m.device, dtype=dtype)
        if front is not None:
            t[:len(front)].copy_(front)
        return t

    def op_args(self, R, S):
        return (*self.ring_args(R, S), self.len, self.spec.size, list(self.spec.thetas), self.lpc, self.flags)

    def results(self):
        """(lpc [n_theta, S, R] float64, host; n_entries [S] of a row live at that step) -- after the op; JlmHipError when the kernel
        flagged a product that is not finite"""
        if int(self.flags.cpu()[0]) & 1:
            raise _lib.JlmHipError("cache_rows_kernel flagged a product h_q . h_i that is not finite: a hidden state is NaN or inf")
        return self.lpc.cpu().numpy().astype(np.float64), self.n_entries()


class CachedScores:
    """What a cached stream call returns.  ``nll_lm`` [B, n] float64: score_streams' result, bit for bit; ``logp_cache``
    [n_theta, B, n] float64: lpc of the kernel's float32 (-inf where nothing matches; unused where ``n_entries`` is 0); ``n_entries``
    [B, n]; ``thetas``; ``h``, ``c``, ``state``: what the next call of the stream carries."""

    def __init__(self, nll_lm, logp_cache, n_entries, thetas, h, c, state):
        self.nll_lm, self.logp_cache, self.n_entries, self.thetas = nll_lm, logp_cache, n_entries, tuple(thetas)
        self.h, self.c, self.state = h, c, state

    def nll(self, lam, theta_index=0):
        """the mixture of the definition at ``lam`` and thetas[theta_index], float64 [B, n]; nll(0) is nll_lm bit for bit"""
        if not is_int(theta_index) or not 0 <= theta_index < len(self.thetas):
            raise ValueError("theta_index must be in [0, %d) (got %r)" % (len(self.thetas), theta_index))
        return mix_nll(self.nll_lm, self.logp_cache[theta_index], self.n_entries, lam)


def score_streams_cached(scorer, inputs, targets, cache, h=None, c=None, state=None):
    """LSTM_Model.score_streams_cached: see there."""
    m = scorer.m
    spec = _check_spec(cache)
    x, y, B, n = check_streams(m, inputs, targets, h, c, "score")
    _check_state(m, state, B)
    n_theta = len(spec.thetas)
    if B == 0 or n == 0:
        return CachedScores(np.zeros((B, n)), np.full((n_theta, B, n), -np.inf), np.zeros((B, n), dtype=np.int64), spec.thetas, h, c, state)
    rings = Rings(m, spec, B, n, [n] * B, state)
    _seq, tok, h2, c2 = scorer.run(x.T, y.T, [B] * n, h=h, c=c, per_token=True, rings=rings)
    lpc, n_entries = rings.results()
    pos = (state.pos if state is not None else 0) + n
    return CachedScores(np.ascontiguousarray(tok.T), np.ascontiguousarray(lpc.transpose(0, 2, 1)),
                        np.ascontiguousarray(np.broadcast_to(n_entries[None, :], (B, n))), spec.thetas, h2, c2, rings.state_after(pos))


def score_cached(scorer, sequences, start, cache, max_rows=None):
    """LSTM_Model.score_cached: see there."""
    m = scorer.m
    spec = _check_spec(cache)

    def run(ch, word, target, lens):
        rings = Rings(m, spec, len(lens), ch["n_steps"], lens)
        tok = scorer.run(word, target, ch["n_live"], per_token=True, rings=rings)[1]
        lpc, n_entries = rings.results()
        return [mix_nll(tok[:n, r], lpc[0, :n, r], n_entries[:n], spec.lam) for r, n in enumerate(lens)]
    return sentence_loop(m, sequences, start, "score", max_rows, (MAX_ROWS, SCORE_BUDGET_BYTES),
                         lambda n: scorer.row_bytes(n, True, spec.size, len(spec.thetas)), lambda n: np.zeros(n, dtype=np.float64), run)


# ---------------------------------------------------------------------------------------------------------------- ranking and prediction
MIX_MAX_SIZE = 4096                 # JLM_CACHE_MIX_MAX_N


def _check_mix_spec(cache):
    """a CacheSpec the mixing loop takes: one theta (a rank depends on lam and theta both) and size <= 4096"""
    spec = _check_spec(cache)
    if len(spec.thetas) != 1:
        raise ValueError("ranking and prediction under the cache take one theta a call (got %d)" % len(spec.thetas))
    if spec.size > MIX_MAX_SIZE:
        raise ValueError("ranking and prediction under the cache take a cache of at most %d entries (got %d)" % (MIX_MAX_SIZE, spec.size))
    return spec


def _check_state(m, state, B):
    if state is not None:
        if not isinstance(state, CacheState) or state.m is not m:
            raise ValueError("this cache state belongs to another model")
        if state.n_rows != B:
            raise ValueError("this cache state holds %d streams, the call has %d" % (state.n_rows, B))


def _flag_error(fl):
    if fl & 1:
        return _lib.JlmHipError("cache_query_kernel flagged a product h_q . h_i that is not finite: a hidden state is NaN or inf")
    if fl & 2:
        return _lib.JlmHipError("cache_mix_rows_kernel flagged a row whose log-normaliser is not finite")
    return _lib.JlmHipError("cache_mix_rows_kernel flagged a cached word outside the vocabulary (flags %d)" % fl)


class MixRings(Ring):
    """The rings of one cached ranking call (jlm_cache_mix_plan): :class:`Ring` in zeroed memory, with the scratch ``s`` [R, N] of one
    step's scores in lpc's place, and ``top`` > 0 the lists top_ids / top_nll [S, R, top] of every step."""
    op = "rank_cache_frames"            # the op Ranker.run calls with op_args behind rank_frames' arguments

    def __init__(self, m, spec, R, S, state=None, top=0):
        torch, dev = m.torch, m.device
        self.top = int(top)
        with m._ctx():
            super().__init__(m, spec, R, S, state)
            self.s = torch.zeros((R, spec.size), device=dev, dtype=torch.float32)
            self.top_ids = torch.full((S, R, self.top), -1, device=dev, dtype=torch.int32) if self.top else None
            self.top_nll = torch.full((S, R, self.top), float("nan"), device=dev, dtype=torch.float64) if self.top else None

    def _slots(self, shape, dtype, front):
        # (no uninitialised memory here: the carried entries and zeros behind them in one pass -- every slot is written before it is
        #  read, DESIGN.md section 19, and the fill is the slots the copy of the carried entries leaves)
        k = len(front) if front is not None else 0
        rest = self.m.torch.zeros((shape[0] - k,) + shape[1:], device=self.m.device, dtype=dtype)
        return rest if front is None else self.m.torch.cat([front, rest])

    @staticmethod
    def row_bytes(H, N, S, top):
        return (N + S) * (4 * H + 4) + 4 * N + 12 * S * top

    def op_args(self, R, S):
        return (*self.ring_args(R, S), self.spec.size, self.spec.theta, self.spec.lam, self.s, self.spec.size, self.top, self.top_ids,
                self.top_nll, self.flags)

    def check(self):
        fl = int(self.flags.cpu()[0])
        if fl:
            raise _flag_error(fl)

    def lists(self, self_norm):
        """(top_ids [S, R, top] int64, top_logp [S, R, top] float64 = log p_q under the mixture) -- after the op"""
        ids = self.top_ids.cpu().numpy().astype(np.int64)
        logp = -self.top_nll.cpu().numpy()
        if self_norm and self.spec.lam > 0:                # y' orders as p_q does; exp(y') sums to 1 / (1 - lam) where the cache has entries
            logp = logp + np.where(self.n_entries() > 0, np.log1p(-float(np.float32(self.spec.lam))), 0.0)[:, None, None]
        return ids, logp


class CachedRanks:
    """What a cached ranking call of streams returns.  ``ranks`` [B, n, columns] int32: rank_streams' array under the mixed
    distribution; ``top_ids`` [B, n, top] int64 / ``top_logp`` [B, n, top] float64 (log p_q, most probable first) when ``top`` > 0,
    else None; ``n_entries`` [B, n]; ``h``, ``c``, ``state``: what the next call of the stream carries (interchangeable with
    score_streams_cached's)."""

    def __init__(self, ranks, top_ids, top_logp, n_entries, h, c, state):
        self.ranks, self.top_ids, self.top_logp, self.n_entries = ranks, top_ids, top_logp, n_entries
        self.h, self.c, self.state = h, c, state


def _check_top(top, V):
    if not is_int(top) or not 0 <= top <= min(64, V):
        raise ValueError("top must be an integer in [0, %d] (got %r)" % (min(64, V), top))
    return int(top)


def rank_streams_cached(ranker, inputs, targets, cache, h=None, c=None, state=None, levels=None, top=0):
    """LSTM_Model.rank_streams_cached: see there."""
    m = ranker.m
    spec = _check_mix_spec(cache)
    top = _check_top(top, m.V)
    x, y, B, n = check_streams(m, inputs, targets, h, c, "rank")
    _check_state(m, state, B)
    L = levels.n_levels if levels is not None else 0
    if B == 0 or n == 0:
        return CachedRanks(np.full((B, n, L + 1), -1, dtype=np.int32), np.zeros((B, n, top), dtype=np.int64) if top else None,
                           np.zeros((B, n, top)) if top else None, np.zeros((B, n), dtype=np.int64), h, c, state)
    rings = MixRings(m, spec, B, n, state, top)
    ranks, h2, c2 = ranker.streams(x, y, h, c, levels, rings)
    ids = logp = None
    if top:
        ids, logp = rings.lists(m.self_norm)
        ids, logp = np.ascontiguousarray(ids.transpose(1, 0, 2)), np.ascontiguousarray(logp.transpose(1, 0, 2))
    pos = (state.pos if state is not None else 0) + n
    return CachedRanks(ranks, ids, logp, np.ascontiguousarray(np.broadcast_to(rings.n_entries()[None, :], (B, n))), h2, c2,
                       rings.state_after(pos))


def rank_cached(ranker, sequences, start, cache, levels=None, max_rows=None):
    """LSTM_Model.rank_cached: see there."""
    return ranker.sentences(sequences, start, levels, max_rows, (MAX_ROWS, GENERATE_BUDGET_BYTES), _check_mix_spec(cache))


def predict_next_cached(ranker, h, state, cache, n=10, allowed=None):
    """LSTM_Model.predict_next_cached: see there."""
    m = ranker.m
    torch = m.torch
    spec = _check_mix_spec(cache)
    if m.mode == "untied" and m.split_lstm:
        raise ValueError("predict_next_cached has no form for an untied split-row model: the f32 copy of the state its vocabulary "
                         "GEMMs read exists only inside the LSTM step")
    if h is None or len(tuple(h.shape)) != 2 or int(h.shape[1]) != m.H:
        raise ValueError("h must be the carried state [B, %d] a stream call returned" % m.H)
    B = int(h.shape[0])
    _check_state(m, state, B)
    if not is_int(n) or not 1 <= n <= min(64, m.V):
        raise ValueError("n must be an integer in [1, %d] (got %r)" % (min(64, m.V), n))
    sets = check_allowed(allowed, B, m.V, "predict_next_cached (allowed)")
    out = [(np.zeros(0, dtype=np.int64), np.zeros(0))] * B
    if B == 0 or (sets is not None and all(s is not None and not len(s) for s in sets)):
        return out
    # the window is the state's last min(count, N) entries: a ring of exactly those, read in place
    cnt = min(state.count, spec.size) if state is not None else 0
    dev, i32 = m.device, torch.int32
    with m._ctx():
        rs = RowSets(m, B, logits=True)
        if cnt:
            hist = state.hist[state.count - cnt:].view(torch.float32).contiguous()
            words = state.words[state.count - cnt:].contiguous()
        else:
            hist = torch.zeros((1, B, m.H), device=dev, dtype=torch.float32)
            words = torch.zeros((1, B), device=dev, dtype=i32)
        N = max(cnt, 1)
        first = torch.zeros(B, device=dev, dtype=i32)
        s = torch.zeros((B, N), device=dev, dtype=torch.float32)
        ids = torch.full((B, n), -1, device=dev, dtype=i32)
        nll = torch.full((B, n), float("nan"), device=dev, dtype=torch.float64)
        cflags = torch.zeros(1, device=dev, dtype=i32)
        mask_args = (None, 0, 0, [])
        if sets is not None:
            restricted = [r for r in range(B) if sets[r] is not None and len(sets[r])]      # (an empty set: no result, below)
            mask, index = ReadingIndex.mask([sets[r] for r in restricted], m.V)
            row_set = [-1] * B
            for r, k in zip(restricted, index):
                row_set[r] = int(k)
            mask_args = (torch.from_numpy(mask.view(np.int32)).to(dev), mask.shape[1], mask.shape[0], row_set)
        hq = h.view(torch.float32).contiguous()
        _ops.backend().predict_cache_rows(m.decode_model(), hq, None if t_is_state(m) else rs.T, rs.logits, rs.ld_logits, rs.rows, hist, words,
                                          N, cnt, first, N, spec.theta, spec.lam, s, N, int(n), *mask_args, ids, nll, rs.flags, cflags, B)
        rs.check_flags("topk_rows_kernel flagged a logit or log-normaliser that is not finite (flags %d)")
        fl = int(cflags.cpu()[0])
        if fl:
            raise _flag_error(fl)
        ids_h, logp = ids.cpu().numpy().astype(np.int64), -nll.cpu().numpy()
    if m.self_norm and spec.lam > 0 and cnt:
        logp = logp + np.log1p(-float(np.float32(spec.lam)))
    res = []
    for r in range(B):
        keep = ids_h[r] >= 0                               # a set smaller than n pads its list with (-1, +inf)
        if sets is not None and sets[r] is not None and not len(sets[r]):
            keep[:] = False
        res.append((ids_h[r][keep], logp[r][keep]))
    return res


# ---------------------------------------------------------------------------------------------------------------- tuning (numpy)
def _as_list(scores):
    return [scores] if isinstance(scores, CachedScores) else list(scores)


def perplexity_grid(scores_by_theta, lams):
    """[n_theta, n_lam] float64: exp(mean nll_mix) over every token of ``scores_by_theta`` -- one :class:`CachedScores` or a list of
    them (the calls of one corpus, all with the same thetas) -- for every theta they carry and every lam of ``lams``"""
    parts = _as_list(scores_by_theta)
    if not parts:
        raise ValueError("no scores to tune on")
    thetas = parts[0].thetas
    if any(p.thetas != thetas for p in parts):
        raise ValueError("every call must carry the same thetas")
    lams = [check_lam(x) for x in lams]
    if not lams:
        raise ValueError("no lam to try")
    n_tok = sum(p.nll_lm.size for p in parts)
    if n_tok == 0:
        raise ValueError("no token to tune on")
    grid = np.zeros((len(thetas), len(lams)))
    for t in range(len(thetas)):
        for j, lam in enumerate(lams):
            grid[t, j] = sum(float(p.nll(lam, t).sum()) for p in parts)
    return np.exp(grid / n_tok)


def tune(scores_by_theta, lams):
    """-> (theta, lam) of the lowest perplexity on the grid thetas x ``lams`` (the first such pair in that order on a tie).  lam is
    swept here, on the host, from the one device pass that made ``scores_by_theta``: lpc does not depend on it."""
    grid = perplexity_grid(scores_by_theta, lams)
    t, j = np.unravel_index(int(np.argmin(grid)), grid.shape)
    return _as_list(scores_by_theta)[0].thetas[t], float(list(lams)[j])
