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
--cache`` the command-line front end.
"""
import numpy as np

from . import _lib
from .rowsets import check_ids, clamp_rows, is_int
from .score import MAX_ROWS, SCORE_BUDGET_BYTES, plan_rows, sentence_arrays

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


class Rings:
    """The rings of one cached call of R rows and S steps (jlm_cache_plan): cap = N + S slots, the carried entries at the local
    positions 0 .. carried - 1 and the call's steps at carried .. carried + S - 1 -- a call numbers positions from its oldest carried
    entry, so ``first`` is 0 and no slot wraps; :class:`CacheState` keeps the stream's own numbering.  ``lens`` [R]: the steps each
    row is live."""

    def __init__(self, m, spec, R, S, lens, state=None):
        torch, dev = m.torch, m.device
        self.m, self.spec, self.R, self.S = m, spec, R, S
        N = spec.size
        self.carried = min(state.count, N) if state is not None else 0
        self.cap = N + S
        with m._ctx():
            self.hist = torch.empty((self.cap, R, m.H), device=dev, dtype=torch.float32)
            self.words = torch.empty((self.cap, R), device=dev, dtype=torch.int32)
            if self.carried:
                self.hist[:self.carried].copy_(state.hist[state.count - self.carried:].view(torch.float32))
                self.words[:self.carried].copy_(state.words[state.count - self.carried:])
            self.first = torch.zeros(R, device=dev, dtype=torch.int32)
            self.len = torch.from_numpy(np.ascontiguousarray(lens, dtype=np.int32)).to(dev)
            self.lpc = torch.full((len(spec.thetas), S, R), float("-inf"), device=dev, dtype=torch.float32)
            self.flags = torch.zeros(1, device=dev, dtype=torch.int32)

    def op_args(self, R, S):
        if (R, S) != (self.R, self.S):
            raise ValueError("these rings were made for %d rows and %d steps (got %d, %d)" % (self.R, self.S, R, S))
        return (self.hist, self.words, self.cap, self.carried, self.first, self.len, self.spec.size, list(self.spec.thetas), self.lpc,
                self.flags)

    def results(self):
        """(lpc [n_theta, S, R] float64, host; n_entries [S] of a row live at that step) -- after the op; JlmHipError when the kernel
        flagged a product that is not finite"""
        if int(self.flags.cpu()[0]) & 1:
            raise _lib.JlmHipError("cache_rows_kernel flagged a product h_q . h_i that is not finite: a hidden state is NaN or inf")
        n_entries = np.minimum(self.carried + np.arange(self.S, dtype=np.int64), self.spec.size)
        return self.lpc.cpu().numpy().astype(np.float64), n_entries

    def state_after(self, pos):
        """the CacheState after the call's S steps (every row live to the end), the stream's next position being ``pos``"""
        end = self.carried + self.S
        cnt = min(end, self.spec.size)
        # (views: the rings are not written after the call, and a copy of N state rows a call costs as much as the cache pass)
        return CacheState(self.m, self.hist[end - cnt:end], self.words[end - cnt:end], pos)


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
    x = np.asarray(inputs)
    y = np.asarray(targets)
    if x.ndim != 2 or x.shape != y.shape:
        raise ValueError("inputs and targets must be [B, n] arrays of the same shape (got %s, %s)" % (x.shape, y.shape))
    if (h is None) != (c is None):
        raise ValueError("carry both h and c, or neither")
    B, n = x.shape
    if state is not None:
        if not isinstance(state, CacheState) or state.m is not m:
            raise ValueError("this cache state belongs to another model")
        if state.n_rows != B:
            raise ValueError("this cache state holds %d streams, the call has %d" % (state.n_rows, B))
    check_ids(x, m.V, "score")
    check_ids(y, m.V, "score")
    if h is not None and (tuple(h.shape) != (B, m.H) or tuple(c.shape) != (B, m.H)):
        raise ValueError("the carried state must be [%d, %d] (got %s, %s)" % (B, m.H, tuple(h.shape), tuple(c.shape)))
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
    seqs = [np.asarray(s, dtype=np.int64).ravel() for s in sequences]
    for s in seqs:
        check_ids(s, m.V, "score")
    check_ids([start], m.V, "score (start)")
    lens = [len(s) for s in seqs]
    longest = max(lens) if lens else 0
    if max_rows is None:
        max_rows = clamp_rows(MAX_ROWS, SCORE_BUDGET_BYTES, scorer.row_bytes(longest, True, spec.size, len(spec.thetas)), m.H)
    out = [np.zeros(L, dtype=np.float64) for L in lens]
    for ch in plan_rows(lens, max_rows):
        idx = ch["idx"]
        word, target = sentence_arrays([seqs[i] for i in idx], start, ch["n_steps"])
        rings = Rings(m, spec, len(idx), ch["n_steps"], ch["lens"])
        _seq, tok, _h, _c = scorer.run(word, target, ch["n_live"], per_token=True, rings=rings)
        lpc, n_entries = rings.results()
        for r, i in enumerate(idx):
            L = int(ch["lens"][r])
            out[i] = mix_nll(tok[:L, r], lpc[0, :L, r], n_entries[:L], spec.lam)
    return out


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
