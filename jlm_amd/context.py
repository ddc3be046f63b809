"""Left context of a conversion: ``LSTM_Model.prime`` and the ``context=`` argument of the decoders.

The reference starts every decode at the zero LSTM state with ``<eos>`` as the only history (decoder/decoder.py:220-241).  An input
method converts in the middle of a text: sentence s with the committed words ``ctx_s`` (word ids; it may be empty and may hold
``<eos>``, as the training stream does) has the history ``hist = [<eos>] + ctx_s``, and its decode is the reference's with two changes
at frame 0: the root hypothesis consumes ``hist[-1]`` instead of ``<eos>``, from the state reached by consuming ``hist[:-1]`` from the
zero state.  Path scores still start at 0, so a score is -log p(path | hist); the context never shows in the output.

Here: :class:`ContextState`, the immutable primed state a caller may hold and reuse; the host planning of a priming call (validation,
rows sorted longest first, right-aligned step arrays, live counts -- the plan of generate's prompt frames, jlm_amd/rowsets.py); and
:class:`Primer`, the row-set driver beside Scorer, Generator and Completer: ONE op (``torch.ops.jlm.prime_frames``, csrc/jlm_decode.hip
``jlm_prime_frames``) that launches the LSTM step of every frame and nothing else.  ``DecodeEngine.submit(context=)`` gathers the rows
of a batch behind its plan's state pool (``torch.ops.jlm.seed_context``, ``seed_context_kernel``) in front of the frame loop.

The continuous cache inside a decode: ``prime(cache=CacheSpec)`` keeps the last N (state, next word) pairs of
every history too (``torch.ops.jlm.prime_cache_frames``) and returns a :class:`CachedContext`; the frame loop then mixes the cache
over that fixed window into every edge cost (csrc/jlm_cache_edge.hip), and the host-side searches do the same in float64
(:meth:`DecodeContext.host_mixer`).
"""
from collections import namedtuple

import numpy as np

from . import ops as _ops
from . import rowsets
from .generate import EOS_ID

# rows per priming call: the gate GEMM's efficient range (jlm_amd/score.py MAX_ROWS); a call's buffers are four state rows a row
MAX_ROWS = 20480
PRIME_BUDGET_BYTES = 1 << 30


class ContextState:
    """The primed state of n histories on the device of a :class:`jlm_amd.model.DeviceModel`; nothing in it is written after it is
    made.  ``h``, ``c`` [n, H]: the state after ``hist[:-1]``, h in the model's state-row format (split rows or f32: 4 bytes a value
    either way); ``last`` [n] int32: ``hist[-1]``, the word the root consumes; ``has`` [n] int32: 0 where the history is ``<eos>``
    alone -- the row never stepped and the root starts from the zero state.  ``last_host`` / ``has_host``: their host copies.
    ``tail_host`` [n, 2] int32 (keyword, optional): the last two words of every history, -1 for "no word" -- what a decode under an
    n-gram mixture starts from (``prime`` records it); a state built without it counts as (-1, last_host)."""

    def __init__(self, m, h, c, last, has, last_host, has_host, *, tail_host=None):
        self.m, self.h, self.c, self.last, self.has = m, h, c, last, has
        self.last_host = np.asarray(last_host, dtype=np.int32)
        self.has_host = np.asarray(has_host, dtype=np.int32)
        self.n = int(self.last_host.shape[0])
        if tail_host is None:
            tail_host = np.stack([np.full(self.n, -1, dtype=np.int32), self.last_host], axis=1)
        self.tail_host = np.asarray(tail_host, dtype=np.int32).reshape(self.n, 2)

    def __len__(self):
        return self.n

    def is_empty(self):
        """every history is ``<eos>`` alone: a decode with this state is today's decode"""
        return not self.has_host.any() and bool((self.last_host == EOS_ID).all())

    def numpy(self):
        """(h, c) [n, H] float32 on the host, split rows decoded (hi + lo, the scale divided out); rows without a state are zero"""
        m = self.m
        c = self.c.detach().cpu().numpy().astype(np.float32)
        raw = self.h.detach().cpu().contiguous().numpy()
        if m.split_lstm:
            sp = raw.view(np.float16).reshape(self.n, m.H // 8, 2, 8).astype(np.float64)
            h = ((sp[:, :, 0, :] + sp[:, :, 1, :]).reshape(self.n, m.H) / float(m.h_scale)).astype(np.float32)
        else:
            h = raw.astype(np.float32)
        keep = self.has_host.astype(bool)[:, None]
        return np.where(keep, h, np.float32(0)), np.where(keep, c, np.float32(0))


class CachedContext(ContextState):
    """A :class:`ContextState` that also holds every row's window for a decode under the continuous cache: the
    last ``count[r]`` = min(len(ctx_r), N) pairs (h_j, hist[j + 1]) of hist = [<eos>] + ctx_r, h_j the state after hist[j].  ``hist``
    [cap, n, H] in the model's state-row format, ``words`` [cap, n] int32, ``count`` [n] int32 (``count_host``: its host copy): row r's
    entries are the slots cap - count[r] .. cap - 1, oldest first; the slots below hold nothing that is read.  ``spec``: the CacheSpec
    it was primed for (one theta).  Immutable and reusable like its base."""

    def __init__(self, m, h, c, last, has, last_host, has_host, hist, words, count, count_host, spec, *, tail_host=None):
        super().__init__(m, h, c, last, has, last_host, has_host, tail_host=tail_host)
        self.hist, self.words, self.count, self.spec = hist, words, count, spec
        self.count_host = np.asarray(count_host, dtype=np.int32)
        self.cap = int(words.shape[0])

    def cache_numpy(self):
        """(h [n, cap, H] float32 with split rows decoded, words [n, cap] int64, count [n]) on the host; row r's window is
        h[r, cap - count[r]:], words[r, cap - count[r]:]"""
        from .cache import decode_rows
        h = decode_rows(self.m, self.hist.view(self.m.torch.float32)).transpose(1, 0, 2)
        return np.ascontiguousarray(h), np.ascontiguousarray(self.words.detach().cpu().numpy().T.astype(np.int64)), self.count_host.copy()


def check_decode_cache(cache):
    """the ``cache=`` of a decode: a CacheSpec of ONE theta and N <= 4096 (JLM_CACHE_MIX_MAX_N); ValueError otherwise"""
    from .cache import CacheSpec, MIX_MAX_SIZE
    if not isinstance(cache, CacheSpec):
        raise ValueError("cache must be a CacheSpec (got %r)" % (cache,))
    if len(cache.thetas) != 1:
        raise ValueError("a decode under the cache takes one theta (got %d)" % len(cache.thetas))
    if cache.size > MIX_MAX_SIZE:
        raise ValueError("a decode under the cache keeps at most %d entries a sentence (got %d)" % (MIX_MAX_SIZE, cache.size))
    return cache


def normalize_contexts(contexts, V, w2i=None, unk=0):
    """``contexts`` -- a list whose items are None, empty, or sequences of word ids / lexicon strings -- as int64 id arrays.  Strings
    go through ``w2i`` (a word outside it is ``unk``, as the lattice maps it).  ValueError for an id outside [0, V), for a string
    without ``w2i``, or for anything else -- before anything runs."""
    if contexts is None or isinstance(contexts, (str, bytes)) or not hasattr(contexts, "__len__"):
        raise ValueError("contexts: a list of word sequences (got %r)" % (type(contexts).__name__,))
    out, plain = [], []
    for i, ctx in enumerate(contexts):
        if ctx is None:
            out.append(np.zeros(0, dtype=np.int64))
            continue
        if isinstance(ctx, (str, bytes)):
            raise ValueError("context %d is a string: a context is a sequence of words" % i)
        a = ctx if isinstance(ctx, np.ndarray) else np.asarray(ctx)
        if a.size == 0 or (a.ndim == 1 and a.dtype.kind in "iu"):          # ids already: no per-word work, one range check for all
            out.append(a.astype(np.int64).ravel())
            plain.append(i)
            continue
        ids = []
        for w in ctx:
            if isinstance(w, str):
                if w2i is None:
                    raise ValueError("context %d holds the string %r: this entry point takes word ids" % (i, w))
                ids.append(int(w2i.get(w, unk)))
            elif rowsets.is_int(w):
                ids.append(int(w))
            else:
                raise ValueError("context %d holds %r: a word is an id or a lexicon string" % (i, w))
        a = np.asarray(ids, dtype=np.int64)
        rowsets.check_ids(a, V, "context %d" % i)
        out.append(a)
    if plain:
        every = np.concatenate([out[i] for i in plain])
        if every.size and (every.min() < 0 or every.max() >= V):
            for i in plain:
                rowsets.check_ids(out[i], V, "context %d" % i)
    return out


def step_words(ctx, eos=EOS_ID):
    """-> (the words priming consumes: hist[:-1], the word the root consumes: hist[-1]) for hist = [eos] + ctx"""
    hist = np.concatenate(([eos], np.asarray(ctx, dtype=np.int64)))
    return hist[:-1], int(hist[-1])


def plan_priming(contexts, max_rows, eos=EOS_ID):
    """The calls of one ``prime``: rows sorted by step count, longest first (stable), at most ``max_rows`` a call
    (rowsets.plan_prompts).  -> list of dict(idx = the caller's context of each row, n_steps = the longest row's steps, n_live
    [n_steps], word / prev [n_steps, R] int32 right-aligned (rowsets.prompt_arrays; prev -1 at a row's first frame), last [R] =
    hist[-1], has [R] = 1 where the row steps at all, target [n_steps, R] = the word each step predicts: hist[j + 1] at the step that
    consumes hist[j], lens [R] = the steps of each row).  A call whose rows never step has n_steps = 0."""
    steps, last = [], []
    for ctx in contexts:
        w, l = step_words(ctx, eos)
        steps.append(w)
        last.append(l)
    chunks = []
    for ch in rowsets.plan_prompts([len(w) for w in steps], max_rows):
        idx = ch["idx"]
        word, prev = rowsets.prompt_arrays([steps[i] for i in idx], ch["n_prompt"])
        # (what each step is scored on under the cache: the next word of the row, hist[-1] at its last step -- hist[1:], right-aligned)
        target, _ = rowsets.prompt_arrays([np.append(steps[i][1:], last[i])[:len(steps[i])] for i in idx], ch["n_prompt"])
        chunks.append(dict(idx=idx, n_steps=ch["n_prompt"], n_live=ch["n_live"], word=word, prev=prev, target=target, lens=ch["lens"],
                           last=np.asarray([last[i] for i in idx], dtype=np.int32), has=(ch["lens"] > 0).astype(np.int32)))
    return chunks


class Primer:
    """The device side of a priming call over a :class:`jlm_amd.model.DeviceModel`."""

    def __init__(self, dev_model):
        self.m = dev_model
        self.torch = dev_model.torch

    def row_bytes(self, n_steps):
        return (4 * self.m.H + self.m.ldt) * 4 + n_steps * 8 + 16

    def run(self, chunk, cap=0):
        """One call over a chunk of :func:`plan_priming`.  -> (h, c) [R, H] device tensors: the set the last frame wrote.  ``cap`` >= 1:
        the states and targets of the last min(cap, n_steps) frames are kept too (``torch.ops.jlm.prime_cache_frames``): -> (h, c, hist
        [k, R, H], words [k, R]), zeroed memory of which frame f's live rows are written."""
        torch, m = self.torch, self.m
        R, S = len(chunk["idx"]), int(chunk["n_steps"])
        rs = rowsets.RowSets(m, R)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(m.device)
        if cap:
            k = max(min(int(cap), S), 1)
            hist = torch.zeros((k, R, m.H), device=m.device, dtype=torch.float32)
            words = torch.zeros((k, R), device=m.device, dtype=torch.int32)
            if S > 0:
                _ops.backend().prime_cache_frames(m.decode_model(), rs.h[0], rs.c[0], rs.h[1], rs.c[1], rs.rows, up(chunk["prev"]),
                                                  up(chunk["word"]), up(chunk["n_live"]), [int(x) for x in chunk["n_live"]], R, S,
                                                  up(chunk["target"]), hist, words, k)
            return rs.h[S % 2], rs.c[S % 2], hist, words
        if S > 0:
            _ops.backend().prime_frames(m.decode_model(), rs.h[0], rs.c[0], rs.h[1], rs.c[1], rs.rows, up(chunk["prev"]), up(chunk["word"]),
                                        up(chunk["n_live"]), [int(x) for x in chunk["n_live"]], R, S)
        return rs.h[S % 2], rs.c[S % 2]


def prime(primer, contexts, max_rows=None, w2i=None, unk=0, checked=False, cache=None):
    """LSTM_Model.prime: see there.  checked: ``contexts`` is what normalize_contexts returned.  cache: a CacheSpec -> a
    :class:`CachedContext` (cap = min(N, the longest context), at least 1)."""
    m = primer.m
    torch = primer.torch
    if cache is not None:
        check_decode_cache(cache)
    ctxs = contexts if checked else normalize_contexts(contexts, m.V, w2i, unk)
    n = len(ctxs)
    longest = max([len(c) for c in ctxs] + [0])
    cap = max(min(cache.size, longest), 1) if cache is not None else 0
    if max_rows is None:
        max_rows = rowsets.clamp_rows(MAX_ROWS, PRIME_BUDGET_BYTES, primer.row_bytes(longest) + cap * (m.H + 1) * 4, m.H)
    last, has = np.full(n, EOS_ID, dtype=np.int32), np.zeros(n, dtype=np.int32)
    with m._ctx():
        h = torch.zeros((n, m.H), device=m.device, dtype=torch.float32)
        c = torch.zeros((n, m.H), device=m.device, dtype=torch.float32)
        if cap:
            hist = torch.zeros((cap, n, m.H), device=m.device, dtype=torch.float32)
            words = torch.zeros((cap, n), device=m.device, dtype=torch.int32)
        for ch in plan_priming(ctxs, max_rows):
            idx = ch["idx"]
            last[idx], has[idx] = ch["last"], ch["has"]
            if ch["n_steps"] == 0:
                continue
            k = int(ch["has"].sum())          # the rows that stepped are a prefix (longest first); the others stay zero
            at = torch.from_numpy(np.ascontiguousarray(idx[:k], dtype=np.int64)).to(m.device)
            if cap:
                hc, cc, hh, ww = primer.run(ch, cap)
                kk = int(ww.shape[0])         # the call's slots are the last kk of the window: priming is right-aligned
                hist[cap - kk:].index_copy_(1, at, hh[:, :k])
                words[cap - kk:].index_copy_(1, at, ww[:, :k])
            else:
                hc, cc = primer.run(ch)
            h.index_copy_(0, at, hc[:k])
            c.index_copy_(0, at, cc[:k])
        dev = lambda a: torch.from_numpy(a.copy()).to(m.device)
        # the last two words of [<eos>] + ctx, -1 where the history is <eos> alone
        tail = np.array([[(int(x[-2]) if len(x) >= 2 else EOS_ID) if len(x) else -1, int(x[-1]) if len(x) else EOS_ID] for x in ctxs],
                        dtype=np.int32).reshape(n, 2)
        if not cap:
            return ContextState(m, h, c, dev(last), dev(has), last, has, tail_host=tail)
        count = np.minimum([len(x) for x in ctxs], cap).astype(np.int32)
        return CachedContext(m, h, c, dev(last), dev(has), last, has, hist, words, dev(count), count, cache, tail_host=tail)


# What a host-side search takes of one input's left context: the primed state read back (h, c [1, H]: from where the root steps), the
# last word of the history (what the root consumes) and, under the continuous cache, mix(pred, h) (DecodeContext.host_mixer), else None
HostContext = namedtuple("HostContext", "h c word mix")


class DecodeContext:
    """What the decoders pass down: a :class:`ContextState` and, per input of the call, its row."""

    def __init__(self, state, rows):
        self.state, self.rows = state, [int(r) for r in rows]
        self._host = self._window = None

    @property
    def cached(self):
        """the decode runs under the continuous cache: a CachedContext with lam > 0 (lam = 0 is the decode without)"""
        return isinstance(self.state, CachedContext) and self.state.spec.lam > 0.0

    def host_mixer(self, i):
        """None, or for input i of a cached decode the host form of the mixture (the float64 definition, jlm_amd/cache.py):
        mix(pred [rows, V], h [rows, H]) -> (1 - lam) pred + lam c(h) over the input's window; an empty window returns pred"""
        if not self.cached:
            return None
        if self._window is None:
            self._window = self.state.cache_numpy()
        hh, ww, cnt = self._window
        r, spec = self.rows[i], self.state.spec
        n = int(cnt[r])
        keys, words = hh[r, hh.shape[1] - n:].astype(np.float64), ww[r, ww.shape[1] - n:]

        def mix(pred, h):
            pred = np.asarray(pred, dtype=np.float64)
            if n == 0:
                return pred
            s = spec.theta * (np.asarray(h, dtype=np.float64) @ keys.T)
            e = np.exp(s - s.max(axis=1, keepdims=True))
            c = np.zeros_like(pred)
            for q in range(pred.shape[0]):
                np.add.at(c[q], words, e[q] / e[q].sum())
            return (1.0 - spec.lam) * pred + spec.lam * c
        return mix

    def tail(self, i):
        """the last words (at most two) of input i's history [<eos>] + context"""
        return [int(x) for x in self.state.tail_host[self.rows[i]] if x >= 0]

    def sub(self, keep):
        return DecodeContext(self.state, [self.rows[i] for i in keep])

    def for_chunk(self, idx):
        """what ``DecodeEngine.submit(context=)`` takes for the chunk of the call's inputs ``idx``"""
        return self.state, [self.rows[j] for j in idx]

    def host(self, i):
        """input i's left context for the host-side searches: HostContext(h [1, H], c [1, H] float64, the last word, mix)"""
        if self._host is None:
            self._host = self.state.numpy()
        r = self.rows[i]
        h, c = self._host
        return HostContext(h[r:r + 1].astype(np.float64), c[r:r + 1].astype(np.float64), int(self.state.last_host[r]), self.host_mixer(i))


def resolve(model, context, n, w2i, single=False, cache=None):
    """The ``context=`` argument of ``decode`` (single) / ``decode_batch`` -> None (every history is ``<eos>`` alone: today's decode)
    or a :class:`DecodeContext` over ``n`` inputs.  Lists are primed here (``model``: the LSTM_Model), with ``cache`` (a CacheSpec,
    lam > 0) into a :class:`CachedContext`.  ValueError for a length mismatch, a bad id, a state of another model, or ``cache=``
    beside a state that was primed already."""
    if cache is not None:
        check_decode_cache(cache)
        if isinstance(context, (DecodeContext, ContextState)):
            raise ValueError("cache=: the context is primed already; prime it with LSTM_Model.prime(contexts, cache=...)")
        if cache.lam == 0.0:
            cache = None                  # p = p_lm: the decode without a cache, the same launches
    if context is None or isinstance(context, DecodeContext):
        return context
    if isinstance(context, ContextState):
        if context.m is not model.dev:
            raise ValueError("context: this ContextState was primed on another model")
        if context.n != n:
            raise ValueError("context: a ContextState of %d rows for %d input(s)" % (context.n, n))
        state = context
    else:
        if single:
            context = [context]
        elif isinstance(context, (str, bytes)) or not hasattr(context, "__len__"):
            raise ValueError("context: one entry per input (None, empty or a word sequence), or a ContextState")
        if len(context) != n:
            raise ValueError("context: %d entries for %d input(s)" % (len(context), n))
        unk = w2i.get("<unk>", 0)
        ctxs = normalize_contexts(context, model.dev.V, w2i, unk)
        if not any(len(c) for c in ctxs):
            return None
        state = prime(model._primer(), ctxs, checked=True, cache=cache)
    if state.is_empty():
        return None
    return DecodeContext(state, range(n))


def split_sentence(words, n_context):
    """The eval harness's split: of a sentence's gold words the first min(n_context, len(words) - 1) are the context, the rest is
    converted.  -> (context words, remaining words); a one-word sentence has no context."""
    k = max(0, min(int(n_context), len(words) - 1))
    return list(words[:k]), list(words[k:])
