"""A memory of hidden states for teacher-forced scoring: the continuous cache's other half (Grave, Cisse, Joulin, "Unbounded cache model
for online language modeling with open vocabulary", NIPS 2017; with exact search, the datastore of a kNN-LM).

The cache of jlm_amd/cache.py lives inside one stream: it starts empty, forgets after N steps and is private to its row.  A memory is
ONE store of (k_i, v_i) pairs -- a hidden state and the word that followed it -- built once from a text, resident on the device, shared
by every row of every call, and saved to disk.  Definition (include/jlm_hip.h): a query position q has the state
h_q and is scored on w_q; for every theta of the call

    s_i       = theta (h_q . k_i)
    lpm_q     = log sum_{i : v_i = w_q} exp(s_i) - log sum_{i < N} exp(s_i)          (-inf when no i matches)
    p_q       = (1 - lam) exp(-nll_q) + lam exp(lpm_q)
    nll_mix_q = -log p_q                                                             (float64, here: cache.mix_nll with n_entries = N)

-- no causality, no window: every query sees every entry.  A call is ONE op (``torch.ops.jlm.score_memory_frames``, csrc/jlm_decode.hip
``jlm_score_memory_frames``): ``score_frames``' launches, the written state rows kept as the call's queries, and ``memory_rows_kernel``
/ ``memory_fold_kernel`` (csrc/jlm_memory.hip) once behind the last step.  lpm does not depend on lam, so lam is swept on the host from
one device pass (:func:`tune`, which is cache.tune).

``LSTM_Model.score_memory`` / ``score_streams_memory`` (jlm_amd/model.py) are the public entry points; ``python -m jlm_amd.memory``
builds and saves a memory from a text, ``python -m jlm_amd.perplexity --memory`` reports the perplexity under one.
"""
import numpy as np

from . import _lib
from . import cache as _cache
from . import ops as _ops
from .cache import CacheSpec, decode_rows, mix_nll
from .rowsets import RowSets, check_streams, is_int, t_is_state
from .score import MAX_ROWS, SCORE_BUDGET_BYTES, sentence_loop

MAX_KEYS = 1 << 24                  # JLM_MEMORY_MAX_KEYS
MIN_SPLIT_KEYS = 512                # JLM_MEMORY_MIN_SPLIT_KEYS
MAX_SPLITS = 128                    # JLM_MEMORY_MAX_SPLITS
TOPK_MAX = 1024                     # JLM_MEMORY_TOPK_MAX
TOPK_SCORE_BYTES = 1 << 28          # the most a retrieval's chunk of scores takes: a smaller memory is one chunk, a larger one several


def keys_per_split(N):
    """jlm_memory_keys_per_split: the keys one workgroup of memory_rows_kernel reads, a function of N alone"""
    return max(MIN_SPLIT_KEYS, -(-(-(-N // MAX_SPLITS)) // 64) * 64)


class MemorySpec:
    """What a call against a memory is asked for: ``theta`` >= 0 -- one value or a sequence of 1 .. 16 for tuning (one device pass
    serves them all) -- and 0 <= ``lam`` < 1.  ValueError for anything else, here, before anything runs."""

    def __init__(self, theta=0.3, lam=0.1):
        spec = CacheSpec(1, theta, lam)              # (the same checks, the same messages)
        self.thetas, self.lam = spec.thetas, spec.lam

    @property
    def theta(self):
        return self.thetas[0]


class MemoryMix:
    """What ranking and prediction under a memory are asked for: the ``memory``, ONE ``theta`` >= 0 (a rank
    depends on theta and lam both), 0 <= ``lam`` < 1 and 1 <= ``k`` <= 1024, the number of nearest entries that vote.  ValueError for
    anything else, here, before anything runs; a memory of another model is refused by the call that is given it."""

    def __init__(self, memory, theta=0.3, lam=0.1, k=64):
        if not isinstance(memory, Memory):
            raise ValueError("memory must be a Memory (got %r)" % (memory,))
        spec = CacheSpec(1, theta, lam)              # (the same checks, the same messages)
        if len(spec.thetas) != 1:
            raise ValueError("ranking and prediction under a memory take one theta a call (got %d)" % len(spec.thetas))
        if not is_int(k) or not 1 <= k <= TOPK_MAX:
            raise ValueError("k must be an integer in [1, %d] (got %r)" % (TOPK_MAX, k))
        self.memory, self.theta, self.lam, self.k = memory, spec.thetas[0], spec.lam, int(k)

    @property
    def n_q(self):
        """the entries that vote: min(k, N)"""
        return min(self.k, self.memory.N)


def _check_mix(m, mix):
    if not isinstance(mix, MemoryMix):
        raise ValueError("mix must be a MemoryMix (got %r)" % (mix,))
    _check_memory(m, mix.memory)
    return mix


def _check_spec(spec):
    if not isinstance(spec, MemorySpec):
        raise ValueError("spec must be a MemorySpec (got %r)" % (spec,))
    return spec


# ---------------------------------------------------------------------------------------------------------------- the definition (float64)
def memory_log_probs(h_q, w_q, keys, key_words, thetas):
    """The definition, in float64.  ``h_q`` [Q, H]: the query states in real units, ``w_q`` [Q]; ``keys`` [N, H], ``key_words`` [N]:
    the memory, decoded.  -> lpm [n_theta, Q] float64, -inf where no entry matches."""
    h = np.asarray(h_q, dtype=np.float64)
    w = np.asarray(w_q)
    k = np.asarray(keys, dtype=np.float64)
    v = np.asarray(key_words)
    th = np.atleast_1d(np.asarray(thetas, dtype=np.float64))
    if k.ndim != 2 or len(k) < 1 or len(k) != len(v) or h.ndim != 2 or h.shape[1] != k.shape[1] or len(h) != len(w):
        raise ValueError("h_q [Q, H] with w_q [Q], keys [N >= 1, H] with key_words [N]")
    lpm = np.full((len(th), len(w)), -np.inf)
    for q in range(len(w)):
        dot = k @ h[q]
        same = v == w[q]
        if not same.any():
            continue
        for t, theta in enumerate(th):
            s = theta * dot
            e = np.exp(s - s.max())
            lpm[t, q] = np.log(e[same].sum()) - np.log(e.sum())
    return lpm


def memory_neighbours(h_q, keys, theta, k):
    """T_K of the definition (include/jlm_hip.h jlm_memory_topk) for ONE query, in float64.  ``h_q`` [H]: the
    query state in real units, ``keys`` [N, H]: the memory, decoded; ``theta`` >= 0; 1 <= ``k`` <= 1024.  -> (idx [n_q] int64, s [n_q]
    float64), n_q = min(k, N): the entries that come first in the order "larger s_i = theta (h_q . k_i) first, smaller i first among
    equal s_i", in that order."""
    h = np.asarray(h_q, dtype=np.float64)
    kv = np.asarray(keys, dtype=np.float64)
    if kv.ndim != 2 or len(kv) < 1 or h.shape != kv.shape[1:]:
        raise ValueError("h_q [H], keys [N >= 1, H]")
    if not is_int(k) or not 1 <= k <= TOPK_MAX:
        raise ValueError("k must be an integer in [1, %d] (got %r)" % (TOPK_MAX, k))
    s = float(theta) * (kv @ h) + 0.0                       # (+ 0: a zero score is +0, one tie)
    idx = np.lexsort((np.arange(len(s)), -s))[:min(int(k), len(s))]       # the last key is the primary one
    return idx.astype(np.int64), s[idx]


def memory_distribution(h_q, keys, key_words, theta, k, V):
    """c_q of the definition for ONE query, in float64: c [V], c(w) = sum_{i in T_K, v_i = w} exp(s_i) / sum_{i in T_K} exp(s_i).
    With k >= N, log c(w_q) is lpm_q of :func:`memory_log_probs`."""
    v = np.asarray(key_words, dtype=np.int64)
    if v.ndim != 1 or len(v) != len(keys) or (len(v) and (v.min() < 0 or v.max() >= V)):
        raise ValueError("key_words [N] inside [0, %d)" % V)
    idx, s = memory_neighbours(h_q, keys, theta, k)
    e = np.exp(s - s.max())
    c = np.zeros(V)
    np.add.at(c, v[idx], e)
    return c / e.sum()


# ---------------------------------------------------------------------------------------------------------------- the store
def _dev_model(model):
    return getattr(model, "dev", model)


def _h_scale(m):
    """the scale of the model's split state rows; f32 rows have none (a model without split rows does not carry the field): 1"""
    return float(m.h_scale) if m.split_lstm else 1.0


class Memory:
    """N (key, word) pairs on the device of a :class:`jlm_amd.model.DeviceModel`; nothing in it is written after it is made.  ``keys``
    [N, H] raw state rows in the model's state-row format (4 bytes a value, viewed as float32), ``words`` [N] int32; ``H``, ``split``,
    ``h_scale``, ``V``: the format fields, the model's."""

    def __init__(self, m, keys, words):
        N = int(words.shape[0])
        if tuple(keys.shape) != (N, m.H) or not 1 <= N <= MAX_KEYS:
            raise ValueError("a memory holds 1 .. %d keys [N, %d] with N words (got %s, %s)" % (MAX_KEYS, m.H, tuple(keys.shape), tuple(words.shape)))
        self.m, self.keys, self.words, self.N = m, keys, words, N
        self.H, self.split, self.h_scale, self.V = int(m.H), bool(m.split_lstm), _h_scale(m), int(m.V)

    def __len__(self):
        return self.N

    @property
    def nbytes(self):
        return self.N * (4 * self.H + 4)

    @classmethod
    def build(cls, model, inputs, targets, num_steps=20):
        """The memory of the streams ``inputs`` / ``targets`` [B, n] (score_streams' arguments, from the zero state): the streams run
        through the scorer in calls of ``num_steps`` steps, state carried, and every step's (h_t, targets[:, t]) is kept in the order
        (call, t, b): N = B n.  The keys are the state rows the LSTM step wrote, as it wrote them."""
        from .cache import Rings
        m = _dev_model(model)
        scorer = model._scorer() if hasattr(model, "_scorer") else None
        if scorer is None:
            from .score import Scorer
            scorer = Scorer(m)
        x, y, B, n = check_streams(m, inputs, targets, None, None, "memory")
        if not is_int(num_steps) or num_steps < 1:
            raise ValueError("num_steps must be an integer >= 1 (got %r)" % (num_steps,))
        if not 1 <= B * n <= MAX_KEYS:
            raise ValueError("a memory holds 1 .. %d entries (got %d x %d)" % (MAX_KEYS, B, n))
        keys, words = [], []
        h = c = None
        store = CacheSpec(1, 0.0, 0.0)             # the ring of a cached call with nothing carried holds the call's rows at its front
        for lo in range(0, n, num_steps):
            S = min(num_steps, n - lo)
            rings = Rings(m, store, B, S, [S] * B)
            _seq, _tok, h, c = scorer.run(x[:, lo:lo + S].T, y[:, lo:lo + S].T, [B] * S, h=h, c=c, per_token=False, rings=rings)
            rings.results()                        # (JlmHipError for a state that is not finite)
            keys.append(rings.hist[:S].reshape(S * B, m.H))
            words.append(rings.words[:S].reshape(S * B))
        with m._ctx():
            return cls(m, m.torch.cat(keys).contiguous(), m.torch.cat(words).contiguous())

    @classmethod
    def concat(cls, a, b):
        """the entries of ``a`` followed by those of ``b`` (memories of one model)"""
        if not isinstance(a, Memory) or not isinstance(b, Memory) or a.m is not b.m:
            raise ValueError("concat joins two memories of one model")
        with a.m._ctx():
            return cls(a.m, a.m.torch.cat([a.keys, b.keys]).contiguous(), a.m.torch.cat([a.words, b.words]).contiguous())

    def save(self, path):
        """an .npz of the raw rows, the words and the four format fields"""
        with open(path, "wb") as f:
            np.savez(f, keys=self.keys.detach().cpu().contiguous().numpy().view(np.uint32), words=self.words.detach().cpu().numpy(),
                     H=np.int64(self.H), split=np.int64(self.split), h_scale=np.float64(self.h_scale), V=np.int64(self.V))

    @classmethod
    def load(cls, model, path):
        """the memory ``save`` wrote, on ``model``'s device.  ValueError when H, split, h_scale or V differ from the model's: the
        rows are raw, and another format reads them as other numbers."""
        m = _dev_model(model)
        with np.load(path) as z:
            missing = [k for k in ("keys", "words", "H", "split", "h_scale", "V") if k not in z.files]
            if missing:
                raise ValueError("%s is not a saved memory (no %s)" % (path, ", ".join(missing)))
            keys, words = z["keys"], z["words"]
            fields = (int(z["H"]), bool(int(z["split"])), float(z["h_scale"]), int(z["V"]))
        want = (int(m.H), bool(m.split_lstm), _h_scale(m), int(m.V))
        for name, got, exp in zip(("H", "split", "h_scale", "V"), fields, want):
            if got != exp:
                raise ValueError("this memory was built with %s = %r, the model has %r" % (name, got, exp))
        if keys.dtype != np.uint32 or keys.ndim != 2 or words.dtype != np.int32 or words.shape != keys.shape[:1]:
            raise ValueError("%s: keys must be uint32 [N, H] and words int32 [N]" % path)
        with m._ctx():
            return cls(m, m.torch.from_numpy(np.ascontiguousarray(keys).view(np.float32)).to(m.device),
                       m.torch.from_numpy(np.ascontiguousarray(words)).to(m.device))

    def numpy(self):
        """(keys [N, H] float32 with split rows decoded, words [N] int64)"""
        return decode_rows(self.m, self.keys), self.words.detach().cpu().numpy().astype(np.int64)

    def search(self, h, k, theta=1.0):
        """The retrieval on its own (jlm_memory_topk): ``h`` [R, H] state rows on the device in the model's state-row format -- what a
        stream call returns, or rows of ``keys`` -- 1 <= ``k`` <= 1024, ``theta`` >= 0.  -> (idx [R, n_q] int64, scores [R, n_q]
        float32, words [R, n_q] int64), n_q = min(k, N): each row's nearest entries, best first, in the order of
        :func:`memory_neighbours`.  JlmHipError when a score is not finite."""
        m = self.m
        torch = m.torch
        mix = MemoryMix(self, theta, 0.0, k)
        if h is None or len(tuple(h.shape)) != 2 or int(h.shape[1]) != m.H or not 0 <= int(h.shape[0]) <= 65535:
            raise ValueError("h must be state rows [R <= 65535, %d] on the device" % m.H)
        R, n_q = int(h.shape[0]), mix.n_q
        if R == 0:
            return np.zeros((0, n_q), dtype=np.int64), np.zeros((0, n_q), dtype=np.float32), np.zeros((0, n_q), dtype=np.int64)
        with m._ctx():
            buf = RetrievalBuffers(m, mix, R)
            _ops.backend().memory_topk(self.keys, self.words, self.N, m.H, self.split, self.h_scale, h.view(torch.float32).contiguous(), R,
                                       mix.theta, mix.k, buf.s, mix.k, buf.ret_words, buf.ret_idx, buf.workspace, buf.flags)
            buf.check()
            return (np.ascontiguousarray(buf.ret_idx[:n_q].cpu().numpy().T.astype(np.int64)), buf.s[:, :n_q].cpu().numpy().copy(),
                    np.ascontiguousarray(buf.ret_words[:n_q].cpu().numpy().T.astype(np.int64)))


def _check_memory(m, memory):
    if not isinstance(memory, Memory) or memory.m is not m:
        raise ValueError("memory must be a Memory of this model")
    return memory


# ---------------------------------------------------------------------------------------------------------------- device side
class MemoryRings:
    """The buffers of one call against a memory (jlm_memory_plan) of R rows and S steps: the query rows q_rows [S, R, H] / q_words
    [S, R], ``lens`` [R] the steps each row is live, lpm [n_theta, S, R] and the workspace of the key split.  The kernels write every
    word of the query rows and the workspace before they read it (tests/test_gpu_memory_rows.py fills both with NaN); they are zeroed
    here all the same -- a few megabytes a call, against a pass over the whole memory."""
    op = "score_memory_frames"           # the op Scorer.run calls with op_args behind score_frames' arguments

    def __init__(self, m, memory, spec, R, S, lens):
        torch, dev = m.torch, m.device
        self.m, self.memory, self.spec, self.R, self.S = m, memory, spec, R, S
        n_theta = len(spec.thetas)
        with m._ctx():
            self.q_rows = torch.zeros((S, R, m.H), device=dev, dtype=torch.float32)
            self.q_words = torch.zeros((S, R), device=dev, dtype=torch.int32)
            self.len = torch.from_numpy(np.ascontiguousarray(lens, dtype=np.int32)).to(dev)
            self.lpm = torch.full((n_theta, S, R), float("-inf"), device=dev, dtype=torch.float32)
            self.workspace = torch.zeros(max(self.workspace_bytes(memory.N, R, S, n_theta) // 4, 1), device=dev, dtype=torch.float32)
            self.flags = torch.zeros(1, device=dev, dtype=torch.int32)

    @staticmethod
    def workspace_bytes(N, R, S, n_theta):
        return int(_lib.lib().jlm_memory_workspace_bytes(int(N), int(R), int(S), int(n_theta)))

    @staticmethod
    def row_bytes(H, N, S, n_theta):
        """bytes a row of a call adds to score's: its S query rows and words, its lpm and its share of the workspace"""
        return S * (4 * H + 4) + 4 * n_theta * S + 12 * n_theta * S * (-(-N // keys_per_split(N))) + 4

    def op_args(self, R, S):
        if (R, S) != (self.R, self.S):
            raise ValueError("these buffers were made for %d rows and %d steps (got %d, %d)" % (self.R, self.S, R, S))
        mem = self.memory
        return (mem.keys, mem.words, mem.N, self.q_rows, self.q_words, self.len, list(self.spec.thetas), self.lpm, self.workspace, self.flags)

    def results(self):
        """lpm [n_theta, S, R] float64, host -- after the op; JlmHipError when the kernel flagged a product that is not finite"""
        if int(self.flags.cpu()[0]) & 1:
            raise _lib.JlmHipError("memory_rows_kernel flagged a product h_q . k_i that is not finite: a hidden state or a key is NaN or inf")
        return self.lpm.cpu().numpy().astype(np.float64)


class MemoryScores:
    """What a stream call against a memory returns.  ``nll_lm`` [B, n] float64: score_streams' result, bit for bit; ``logp_memory``
    [n_theta, B, n] float64: lpm of the kernel's float32 (-inf where no entry matches); ``n_entries``: N; ``thetas``; ``h``, ``c``:
    what the next call of the stream carries."""

    def __init__(self, nll_lm, logp_memory, n_entries, thetas, h, c):
        self.nll_lm, self.logp_memory, self.n_entries, self.thetas = nll_lm, logp_memory, int(n_entries), tuple(thetas)
        self.h, self.c = h, c

    def nll(self, lam, theta_index=0):
        """the mixture of the definition at ``lam`` and thetas[theta_index], float64 [B, n]; nll(0) is nll_lm bit for bit"""
        if not is_int(theta_index) or not 0 <= theta_index < len(self.thetas):
            raise ValueError("theta_index must be in [0, %d) (got %r)" % (len(self.thetas), theta_index))
        return mix_nll(self.nll_lm, self.logp_memory[theta_index], self.n_entries, lam)


def score_streams_memory(scorer, inputs, targets, memory, spec, h=None, c=None):
    """LSTM_Model.score_streams_memory: see there."""
    m = scorer.m
    spec = _check_spec(spec)
    memory = _check_memory(m, memory)
    x, y, B, n = check_streams(m, inputs, targets, h, c, "score")
    n_theta = len(spec.thetas)
    if B == 0 or n == 0:
        return MemoryScores(np.zeros((B, n)), np.full((n_theta, B, n), -np.inf), memory.N, spec.thetas, h, c)
    rings = MemoryRings(m, memory, spec, B, n, [n] * B)
    _seq, tok, h2, c2 = scorer.run(x.T, y.T, [B] * n, h=h, c=c, per_token=True, rings=rings)
    lpm = rings.results()
    return MemoryScores(np.ascontiguousarray(tok.T), np.ascontiguousarray(lpm.transpose(0, 2, 1)), memory.N, spec.thetas, h2, c2)


def score_memory(scorer, sequences, start, memory, spec, max_rows=None):
    """LSTM_Model.score_memory: see there."""
    m = scorer.m
    spec = _check_spec(spec)
    memory = _check_memory(m, memory)
    n_theta = len(spec.thetas)

    def run(ch, word, target, lens):
        rings = MemoryRings(m, memory, spec, len(lens), ch["n_steps"], lens)
        tok = scorer.run(word, target, ch["n_live"], per_token=True, rings=rings)[1]
        lpm = rings.results()
        return [mix_nll(tok[:n, r], lpm[0, :n, r], memory.N, spec.lam) for r, n in enumerate(lens)]
    return sentence_loop(m, sequences, start, "score", max_rows, (MAX_ROWS, SCORE_BUDGET_BYTES),
                         lambda n: scorer.row_bytes(n, True) + MemoryRings.row_bytes(m.H, memory.N, n, n_theta),
                         lambda n: np.zeros(n, dtype=np.float64), run)


# ---------------------------------------------------------------------------------------------------------------- ranking and prediction
def _flag_error(fl):
    if fl & 1:
        return _lib.JlmHipError("the retrieval flagged a score theta (h_q . k_i) that is not finite: a hidden state or a key is NaN or inf")
    if fl & 2:
        return _lib.JlmHipError("cache_mix_rows_kernel flagged a row whose log-normaliser is not finite")
    return _lib.JlmHipError("cache_mix_rows_kernel flagged a word of the memory outside the vocabulary (flags %d)" % fl)


class RetrievalBuffers:
    """The buffers of a retrieval over R rows (jlm_memory_topk's): the scores s [R, K], ret_words / ret_idx [K, R] -- ``steps`` > 0:
    ret_idx [steps, K, R], every step's neighbours kept --, ``first`` [R] zeros (the patch reads the retrieved entries as a window that
    starts at position 0), the workspace and the flag word.  All zeroed, none uninitialised.  Constructed inside the model's context."""

    def __init__(self, m, mix, R, steps=0):
        torch, dev, K = m.torch, m.device, mix.k
        self.m, self.mix, self.R = m, mix, R
        self.s = torch.zeros((R, K), device=dev, dtype=torch.float32)
        self.ret_words = torch.zeros((K, R), device=dev, dtype=torch.int32)
        self.ret_idx = torch.full(((steps, K, R) if steps else (K, R)), -1, device=dev, dtype=torch.int32)
        self.first = torch.zeros(R, device=dev, dtype=torch.int32)
        self.workspace = torch.zeros(max(self.workspace_floats(mix.memory.N, R, K), 4), device=dev, dtype=torch.float32)
        self.flags = torch.zeros(1, device=dev, dtype=torch.int32)

    @staticmethod
    def chunk_keys(N, R):
        """keys per chunk of the retrieval: the whole memory when its scores fit TOPK_SCORE_BYTES, else as many tiles as do"""
        whole = -(-N // 32) * 32
        return max(32, min(whole, TOPK_SCORE_BYTES // (4 * max(R, 1)) // 32 * 32))

    @classmethod
    def workspace_floats(cls, N, R, K):
        return R * (cls.chunk_keys(N, R) + 2 * K)

    @staticmethod
    def row_bytes(N, K, S, top, neighbours):
        """bytes a row of a ranking call adds to rank's: scores, words, indices, its share of the workspace (a chunk of at most the
        whole memory: the row plan has not fixed R yet) and the lists"""
        return 4 * K * (2 + (S if neighbours else 1)) + 4 * min(-(-N // 32) * 32, 1 << 16) + 8 * K + 12 * S * top + 8

    def check(self):
        fl = int(self.flags.cpu()[0])
        if fl:
            raise _flag_error(fl)


class MixBuffers(RetrievalBuffers):
    """... of one ranking call of R rows and S steps (jlm_memory_mix_plan), as the plug Ranker.run takes: with ``top`` > 0 the lists
    top_ids / top_nll [S, R, top] of every step, with ``neighbours`` every step's indices."""
    op = "rank_memory_frames"           # the op Ranker.run calls with op_args behind rank_frames' arguments

    def __init__(self, m, mix, R, S, top=0, neighbours=False):
        torch, dev = m.torch, m.device
        self.S, self.top, self.keep = S, int(top), bool(neighbours)
        with m._ctx():
            super().__init__(m, mix, R, S if neighbours else 0)
            self.top_ids = torch.full((S, R, self.top), -1, device=dev, dtype=torch.int32) if self.top else None
            self.top_nll = torch.full((S, R, self.top), float("nan"), device=dev, dtype=torch.float64) if self.top else None

    def op_args(self, R, S):
        if (R, S) != (self.R, self.S):
            raise ValueError("these buffers were made for %d rows and %d steps (got %d, %d)" % (self.R, self.S, R, S))
        mix, mem = self.mix, self.mix.memory
        return (mem.keys, mem.words, mem.N, mix.theta, mix.lam, mix.k, self.s, mix.k, self.ret_words, self.ret_idx, self.keep, self.first,
                self.workspace, self.top, self.top_ids, self.top_nll, self.flags)

    def lists(self, self_norm):
        """(top_ids [S, R, top] int64, top_logp [S, R, top] float64 = log p_q under the mixture) -- after the op"""
        ids = self.top_ids.cpu().numpy().astype(np.int64)
        logp = -self.top_nll.cpu().numpy()
        if self_norm and self.mix.lam > 0:                 # y' orders as p_q does; exp(y') sums to 1 / (1 - lam): a memory is never empty
            logp = logp + np.log1p(-float(np.float32(self.mix.lam)))
        return ids, logp

    def neighbour_indices(self):
        """[S, R, n_q] int64 -- after the op"""
        return np.ascontiguousarray(self.ret_idx[:, :self.mix.n_q].cpu().numpy().transpose(0, 2, 1).astype(np.int64))


class MemoryRanks:
    """What a ranking call of streams under a memory returns.  ``ranks`` [B, n, columns] int32: rank_streams' array under the mixed
    distribution; ``top_ids`` [B, n, top] int64 / ``top_logp`` [B, n, top] float64 (log p_q, most probable first) when ``top`` > 0,
    else None; ``neighbours`` [B, n, n_q] int64 indices into the memory, best first, or None; ``h``, ``c``: what the next call of the
    stream carries."""

    def __init__(self, ranks, top_ids, top_logp, neighbours, h, c):
        self.ranks, self.top_ids, self.top_logp, self.neighbours, self.h, self.c = ranks, top_ids, top_logp, neighbours, h, c


def rank_streams_memory(ranker, inputs, targets, mix, h=None, c=None, levels=None, top=0, neighbours=False):
    """LSTM_Model.rank_streams_memory: see there."""
    m = ranker.m
    mix = _check_mix(m, mix)
    top = _cache._check_top(top, m.V)
    x, y, B, n = check_streams(m, inputs, targets, h, c, "rank")
    L = levels.n_levels if levels is not None else 0
    if B == 0 or n == 0:
        return MemoryRanks(np.full((B, n, L + 1), -1, dtype=np.int32), np.zeros((B, n, top), dtype=np.int64) if top else None,
                           np.zeros((B, n, top)) if top else None, np.zeros((B, n, mix.n_q), dtype=np.int64) if neighbours else None, h, c)
    buf = MixBuffers(m, mix, B, n, top, neighbours)
    ranks, h2, c2 = ranker.streams(x, y, h, c, levels, buf)
    ids = logp = None
    if top:
        ids, logp = buf.lists(m.self_norm)
        ids, logp = np.ascontiguousarray(ids.transpose(1, 0, 2)), np.ascontiguousarray(logp.transpose(1, 0, 2))
    nb = np.ascontiguousarray(buf.neighbour_indices().transpose(1, 0, 2)) if neighbours else None
    return MemoryRanks(ranks, ids, logp, nb, h2, c2)


def rank_memory(ranker, sequences, start, mix, levels=None, max_rows=None):
    """LSTM_Model.rank_memory: see there."""
    from .generate import GENERATE_BUDGET_BYTES
    m = ranker.m
    mix = _check_mix(m, mix)
    return ranker.sentences(sequences, start, levels, max_rows, (MAX_ROWS, GENERATE_BUDGET_BYTES),
                            patch=lambda word: MixBuffers(m, mix, int(np.shape(word)[1]), int(np.shape(word)[0])),
                            extra_bytes=lambda n: RetrievalBuffers.row_bytes(mix.memory.N, mix.k, n, 0, False))


def predict_next_memory(ranker, h, mix, n=10, allowed=None):
    """LSTM_Model.predict_next_memory: see there."""
    from .complete import check_allowed
    from .readings import ReadingIndex
    m = ranker.m
    torch = m.torch
    mix = _check_mix(m, mix)
    if m.mode == "untied" and m.split_lstm:
        raise ValueError("predict_next_memory has no form for an untied split-row model: the f32 copy of the state its vocabulary "
                         "GEMMs read exists only inside the LSTM step")
    if h is None or len(tuple(h.shape)) != 2 or int(h.shape[1]) != m.H:
        raise ValueError("h must be the carried state [B, %d] a stream call returned" % m.H)
    B = int(h.shape[0])
    if not is_int(n) or not 1 <= n <= min(64, m.V):
        raise ValueError("n must be an integer in [1, %d] (got %r)" % (min(64, m.V), n))
    sets = check_allowed(allowed, B, m.V, "predict_next_memory (allowed)")
    out = [(np.zeros(0, dtype=np.int64), np.zeros(0))] * B
    if B == 0 or (sets is not None and all(s is not None and not len(s) for s in sets)):
        return out
    dev, i32, mem = m.device, torch.int32, mix.memory
    with m._ctx():
        rs = RowSets(m, B, logits=True)
        buf = RetrievalBuffers(m, mix, B)
        ids = torch.full((B, n), -1, device=dev, dtype=i32)
        nll = torch.full((B, n), float("nan"), device=dev, dtype=torch.float64)
        mask_args = (None, 0, 0, [])
        if sets is not None:
            restricted = [r for r in range(B) if sets[r] is not None and len(sets[r])]      # (an empty set: no result, below)
            mask, index = ReadingIndex.mask([sets[r] for r in restricted], m.V)
            row_set = [-1] * B
            for r, k in zip(restricted, index):
                row_set[r] = int(k)
            mask_args = (torch.from_numpy(mask.view(np.int32)).to(dev), mask.shape[1], mask.shape[0], row_set)
        hq = h.view(torch.float32).contiguous()
        _ops.backend().predict_memory_rows(m.decode_model(), hq, None if t_is_state(m) else rs.T, rs.logits, rs.ld_logits, rs.rows, mem.keys,
                                           mem.words, mem.N, mix.theta, mix.lam, mix.k, buf.s, mix.k, buf.ret_words, buf.ret_idx, buf.first,
                                           buf.workspace, int(n), *mask_args, ids, nll, rs.flags, buf.flags, B)
        rs.check_flags("topk_rows_kernel flagged a logit or log-normaliser that is not finite (flags %d)")
        buf.check()
        ids_h, logp = ids.cpu().numpy().astype(np.int64), -nll.cpu().numpy()
    if m.self_norm and mix.lam > 0:
        logp = logp + np.log1p(-float(np.float32(mix.lam)))
    res = []
    for r in range(B):
        keep = ids_h[r] >= 0                               # a set smaller than n pads its list with (-1, +inf)
        if sets is not None and sets[r] is not None and not len(sets[r]):
            keep[:] = False
        res.append((ids_h[r][keep], logp[r][keep]))
    return res


# ---------------------------------------------------------------------------------------------------------------- tuning (numpy)
def perplexity_grid(scores_by_theta, lams):
    """cache.perplexity_grid over one :class:`MemoryScores` or a list of them: [n_theta, n_lam] float64"""
    return _cache.perplexity_grid([scores_by_theta] if isinstance(scores_by_theta, MemoryScores) else scores_by_theta, lams)


def tune(scores_by_theta, lams):
    """cache.tune over one :class:`MemoryScores` or a list of them: -> (theta, lam) of the lowest perplexity on the grid"""
    return _cache.tune([scores_by_theta] if isinstance(scores_by_theta, MemoryScores) else scores_by_theta, lams)


# ---------------------------------------------------------------------------------------------------------------- command line
def main(argv=None):
    """``python -m jlm_amd.memory --root R -e ID --text FILE [-b B --num_steps S] --out MEM.npz``: build the memory of a text -- the
    encoded file as one id stream, laid out as ``python -m jlm_amd.perplexity --mode stream`` lays it out -- and save it."""
    import argparse

    from . import config as _config
    from .data import load_vocab
    ap = argparse.ArgumentParser(description="Build a memory of hidden states from a text and save it (jlm_amd/memory.py)")
    _config.add_model_args(ap)
    ap.add_argument("--text", required=True, help="the text to remember, one sentence per line")
    ap.add_argument("-b", "--batch_size", type=int, default=None, help="parallel streams (default: the config's, else 64)")
    ap.add_argument("--num_steps", type=int, default=20, help="steps per call")
    ap.add_argument("--out", required=True, help="the .npz to write")
    args = ap.parse_args(argv)
    if args.num_steps < 1 or (args.batch_size is not None and args.batch_size < 1):
        ap.error("-b and --num_steps take integers >= 1")
    config, vocab = load_vocab(args)
    from .model import LSTM_Model
    from .perplexity import encode_lines, read_lines
    from .score import stream_layout
    sents, _n_unk = encode_lines(read_lines(args.text), vocab)
    model = LSTM_Model(experiment_id=args.experiment_id, comp=args.comp)
    bs = args.batch_size or int(config.get("batch_size", 64))
    try:
        x, y = stream_layout([i for s in sents for i in s], bs, args.num_steps)
        memory = Memory.build(model, x, y, args.num_steps)
    except ValueError as e:
        ap.error(str(e))
    memory.save(args.out)
    print("memory: N {}  H {}  bytes {}  -> {}".format(memory.N, memory.H, memory.nbytes, args.out))
    return memory


if __name__ == "__main__":
    main()
