"""Lattice Viterbi beam-search decoder on MI355X, reference-compatible API.

Counterpart of ``Decoder`` in the reference (decoder/decoder.py:54-241):

    Decoder(experiment_id=0, comp=0)
    .decode(input, topN=10, beam_width=10, vocab_select=False, samples=0,
            top_sampling=False, random_sampling=False) -> [(neg_log_prob, [word, ...])]
    ._check_oov(word)
    attrs .perf_sen .perf_log_lstm .perf_log_softmax .lattice_vocab
          .backward_lookup .model .w2i .i2w .config

plus ``decode_batch(list_of_inputs, ...)`` (the reference decodes one sentence
at a time; batching sentences is what fills the GPU).  ``decode`` is
``decode_batch`` of one sentence.

``perf_timing`` (default False): with True every frame is bracketed by HIP events
(per-call lists ``perf_log_lstm`` / ``perf_log_softmax`` as the reference fills
them, decoder.py:206-218) and the launches are enqueued one by one from Python on
one stream; the default keeps the native frame loop and the two alternating
streams.  ``jlm_amd.eval`` and the ``compat/`` shims for the reference's
``eval.py`` (which prints those lists) switch it on.

``beam_width=None`` (decoder.py:227: no pruning, the frame keeps every candidate, exponential in the
input length) runs the reference's own loop on the host over ``LSTM_Model.predict_with_context``
(:meth:`Decoder._decode_unpruned`) for as long as a frame holds at most ``max_unpruned_paths``
hypotheses; the result is unsorted, as in the reference.

``compat_quirks = True`` reproduces the stale ``lattice_vocab`` (decoder.py:62,176: once a call with
``vocab_select=True`` has run, later calls without it still normalise over that old list and fail
with ValueError when a word is not in it); off by default.

Deliberate differences (DESIGN.md "Reference quirks"):
  * the LSTM step of the last frame is skipped (its result is never read,
    decoder.py:233-237).
"""
import gc
import os
import pickle
from collections import deque, namedtuple

from . import config as _config
from .data import Vocab
from .engine import DecodeEngine
from .lattice import BatchLattice, LatticeBuilder
from .model import LSTM_Model


class Node():
    """Lattice node view, field names of the reference (decoder.py:17-27)."""

    def __init__(self, s, l, idx, word, oov_prob=0.0):
        self.start_idx = s
        self.reading_length = l
        self.word_idx = idx
        self.word = word
        self.oov_prob = oov_prob
        self.char_rnn_step = 0

    def __repr__(self):
        return str((self.start_idx, self.word))


class _CellTooLarge(Exception):
    """raised by a chunk's preparation: these input indices have a lattice cell the device beam step cannot hold"""

    def __init__(self, sentences):
        Exception.__init__(self, sentences)
        self.sentences = list(sentences)


# a chunk of a call between its preparation and its launch: the call's input indices, their lattice, and what the decode's own ``extra``
# made of the two (word lists, spans; None without one)
_Chunk = namedtuple("_Chunk", "idx lat extra")


class Decoder():
    dynamic = False
    char_model = False           # the class decodes character models (config['char_rnn']): CharRNNDecoder
    # jlm_beam_step keeps the candidates of one (frame, sentence) cell -- nodes ending there x beam -- in one wave's LDS: 12 bytes
    # each of 160 KB, less what the beam and the frame count take (jlm_beam_step_max_cands: the launcher's own formula).
    # Sentences with a larger cell (hundreds of homophones at a wide beam) take the host-side search (_decode_unpruned with the
    # beam; DynamicDecoder._decode_host) instead of failing the batch.  CAND_LIMIT: an explicit limit instead (tests).
    CAND_LIMIT = None
    MAX_BEAM = 1024              # JLM_MAX_BEAM (include/jlm_hip.h); the reference has no limit (decoder.py:227-229)

    def __init__(self, experiment_id=0, comp=0, device=None):
        self.config = _config.load_config_dict(experiment_id)
        if self.config.get('char_rnn') and not self.char_model:
            raise ValueError("experiment %r is a character model (config['char_rnn']): its softmax runs over characters, decode it with "
                             "CharRNNDecoder (jlm_amd/decoder_char.py; reference decoder/eval.py:43-44)" % (experiment_id,))
        self._load_vocab()
        with open(os.path.join(_config.root_path, 'data', 'lexicon.pkl'), 'rb') as f:
            self.full_lexicon = pickle.load(f)
        with open(os.path.join(_config.root_path, 'data', 'reading_dict.pkl'), 'rb') as f:
            self.full_reading_dict = pickle.load(f)
        self.model = LSTM_Model(experiment_id, comp, device=device)
        self._builder = LatticeBuilder(self.full_lexicon, self.full_reading_dict, self.w2i)
        self._engine = DecodeEngine(self.model.dev)
        self.pipeline_depth = self._engine.n_streams      # chunks in flight in decode_batch (see depth_for)
        self._paths_calibrated = False
        self.lattice_vocab = None
        self.backward_lookup = None
        self.perf_sen = 0
        self.perf_log_lstm = []
        self.perf_log_softmax = []
        self.compat_quirks = False       # True: the stale lattice_vocab of decoder.py:62,176 (module docstring)
        self.max_unpruned_paths = 20000  # beam_width=None: largest frame the host-side unpruned search accepts
        self.perf_timing = False         # True: per-frame HIP-event timings into perf_log_* (eval.py reads them), slower path
        self.max_batch = 1024            # sentences per device batch; longer inputs are pipelined in chunks
        self.plan_budget_bytes = 6 << 30  # state rows of one batch (frames x sentences x beam x (2 H + ldt) x 4 B): see _chunks
        self.last_lattice = None
        # (rounds 2-4 could finish or enqueue chunks on a thread of their own -- JLM_COLLECTOR / JLM_SUBMIT_THREAD; measured in
        #  rounds 2, 4 and 5, never a gain -- profiles/r04_a_submit_thread_ab.txt, r05_k_host_bench.txt -- and removed in round 5: the
        #  enqueue is ONE op without the interpreter lock now, engine._enqueue)
        self._pool = None                # worker threads that build the lattices of upcoming chunks
        from . import usable_cpus
        # lattice builds (single-threaded, 1.4 ms per 256-sentence chunk) running ahead of the GPU: two workers keep it fed
        # (tools/probes/e2e_threads.py: 2 workers x 1 thread = 3 x 4 = 2.8-3.0 ms per step, 1 worker 3.4-3.9), three when the
        # process has CPUs to spare
        # (round 3: four or five workers on the 16-CPU box are SLOWER for every decoder kind -- 1.64 / 1.77 vs 1.48 ms per step
        # with vocab_select, tools/probes/host_profile2.py: they contend with the calling thread; JLM_PREFETCH_WORKERS overrides)
        self.prefetch_workers = int(os.environ.get("JLM_PREFETCH_WORKERS", "0")) or (
            3 if usable_cpus() >= 12 else 2)
        self._pool1 = None
        # The lexicon, the reading dictionary and the trie are a few million long-lived Python objects;
        # left in the collector's youngest-to-oldest scan they cost a ~70 ms full collection every ~20
        # batches (tools/probes/stall_probe.py).  Park them in the permanent generation.
        # Process-wide side effect, opt-out: JLM_NO_GC_FREEZE=1 (INTEGRATION.md "process-global knobs").
        if os.environ.get("JLM_NO_GC_FREEZE", "0") != "1":
            gc.collect()
            gc.freeze()
        self._calibrate_on_decoded_paths()

    CALIB_SENTENCES, CALIB_WORDS, CALIB_BEAM = 32, 6, 8

    def _calibrate_on_decoded_paths(self):
        """Round 6 (verdict item 3): the load-time calibration of the normaliser's row format once more on contexts the lattice search
        really visits.  The model alone (DeviceModel._calibrate_mixed) probes seeded word draws; here a few synthetic sentences of
        THIS lexicon -- readings of in-vocabulary words drawn ~ 1 / rank, concatenated -- are decoded, and the word sequences of the
        hypotheses the beam kept become one more probe (DeviceModel.calibrate_on_paths: the worst probe decides).  Only for a model
        that kept mixed rows (a model on split rows has nothing to re-decide); JLM_CALIB_PATHS=0: off."""
        m = self.model.dev
        if self._paths_calibrated or os.environ.get("JLM_CALIB_PATHS", "1") == "0" or m.mixed is None \
                or float(os.environ.get("JLM_MIXED_MAX_LSE_RMS", "1")) <= 0.0:
            return
        self._paths_calibrated = True
        import numpy as np
        rng = np.random.RandomState(20240929)
        V = len(self.w2i)
        sents = []
        for _ in range(self.CALIB_SENTENCES):
            ids = np.minimum((np.exp(rng.random_sample(self.CALIB_WORDS) * np.log(V + 1.0)) - 1.0).astype(np.int64), V - 1)
            reading = ""
            for i in ids:
                tok = self.i2w[int(i)].split("/")
                if len(tok) >= 3:
                    reading += tok[1] if tok[1] != "" else tok[0]
            if reading:
                sents.append(reading[:24])
        if not sents:
            return
        timing, self.perf_timing = self.perf_timing, False
        try:
            nbest = Decoder.decode_batch(self, sents, topN=self.CALIB_BEAM, beam_width=self.CALIB_BEAM)
        except Exception:                  # (a lexicon whose readings do not decode: the synthetic draws stand)
            self.perf_timing = timing
            return
        self.perf_timing = timing
        self.perf_sen = 0
        unk = self.w2i.get("<unk>", 0)
        paths = [[self.w2i.get(w, unk) for w in words] for res in nbest for _s, words in res if words]
        before = m.mixed
        m.calibrate_on_paths(paths, first_word=self.w2i.get("<eos>", 0))
        if (m.mixed_fmt, m.mixed_idx) != (before.fmt, before.idx):
            self._engine = DecodeEngine(m)     # (plans of the form the model had are of no use to the one it has now)
            self.pipeline_depth = self._engine.n_streams
        self.lattice_vocab, self.backward_lookup, self.last_lattice = None, None, None

    def _load_vocab(self):
        self.vocab = Vocab(self.config['vocab_size'])
        self.i2w = self.vocab.i2w
        self.w2i = self.vocab.w2i

    def _check_oov(self, word):
        return word not in self.w2i

    def _build_lattice(self, input, vocab_select=False, samples=0, top_sampling=False, random_sampling=False):
        """Single-sentence lattice in the reference's shape: dict frame -> [Node]
        (decoder.py:79-135)."""
        lat = BatchLattice(self._builder, [input], 1)
        bl = {}
        for f, nodes in enumerate(lat.backward_lookup(0)):
            bl[f] = [Node(s, l, w, word) for (s, l, w, word) in nodes]
        return bl

    def _log_perf(self):
        if self.perf_timing and self._engine.last_timing:
            for t_lstm, t_soft in self._engine.last_timing:
                self.perf_log_lstm.append(t_lstm)
                self.perf_log_softmax.append(t_soft)

    def _context(self, context, n, cache=None):
        """the ``context=`` argument of a batch method (a one-input call's as _Single) as None or a jlm_amd.context.DecodeContext over
        the call's n inputs; ``cache``: the call's CacheSpec (word lists are primed with it)"""
        from . import context as _context
        if cache is not None:
            _context.check_decode_cache(cache)
        single = isinstance(context, _Single)
        if single:
            context = context.context
        if context is None:
            return None
        return _context.resolve(self.model, context, n, self.w2i, single=single, cache=cache)

    def _refuse_cache(self, ctx, what, cache=None):
        """ValueError where a decode under the continuous cache is asked of an entry point or an argument that has none: ``ctx`` the
        call's ``context=`` as given, ``cache`` its CacheSpec -- checked BEFORE the context is resolved, which primes word lists on the
        device"""
        from .context import CachedContext, DecodeContext, check_decode_cache
        if isinstance(ctx, _Single):
            ctx = ctx.context
        state = ctx.state if isinstance(ctx, DecodeContext) else ctx
        if (cache is not None and check_decode_cache(cache).lam > 0.0) or (isinstance(state, CachedContext) and state.spec.lam > 0.0):
            raise ValueError("%s takes no continuous cache (DESIGN.md section 21: the static full-vocabulary Decoder.decode only)" % what)

    def _check_ngram(self, ngram, context, cache, vocab_select):
        """the ``ngram=`` of a decode, checked BEFORE the context is resolved (which primes word lists on the device): an NGramMix whose
        ids lie below the model's V, without ``cache=`` / a CachedContext, ``vocab_select`` or ``compat_quirks``; ValueError otherwise"""
        from .context import CachedContext, DecodeContext
        from .ngram import check_mix
        check_mix(ngram, len(self.w2i))
        if isinstance(context, _Single):
            context = context.context
        state = context.state if isinstance(context, DecodeContext) else context
        if cache is not None or isinstance(state, CachedContext):
            raise ValueError("ngram= and the continuous cache in one decode: a three-way mixture is not defined (DESIGN.md section 24)")
        if vocab_select:
            raise ValueError("vocab_select takes no n-gram mixture (DESIGN.md section 24: the static full-vocabulary Decoder.decode only)")
        if self.compat_quirks:
            raise ValueError("compat_quirks takes no n-gram mixture (DESIGN.md section 24)")
        return ngram

    def _check_memory(self, memory, context, cache, ngram, vocab_select):
        """the ``memory=`` of a decode, checked BEFORE the context is resolved (which primes word lists on the device): a MemoryMix of
        this model (its H and row format), without ``cache=`` / a CachedContext, ``ngram=``, ``vocab_select`` or ``compat_quirks``;
        ValueError otherwise.  -> the MemoryMix, or None for lam = 0: the decode without a memory"""
        from .context import CachedContext, DecodeContext
        from .memory import _check_mix
        _check_mix(self.model.dev, memory)
        if isinstance(context, _Single):
            context = context.context
        state = context.state if isinstance(context, DecodeContext) else context
        if cache is not None or isinstance(state, CachedContext) or ngram is not None:
            raise ValueError("memory= beside the continuous cache or an n-gram mixture: a three-way mixture is not defined (DESIGN.md section 30)")
        if vocab_select:
            raise ValueError("vocab_select takes no memory (DESIGN.md section 30: the static full-vocabulary Decoder.decode only)")
        if self.compat_quirks:
            raise ValueError("compat_quirks takes no memory (DESIGN.md section 30)")
        return memory if memory.lam > 0.0 else None

    def decode_batch(self, inputs, topN=10, beam_width=10, vocab_select=False, samples=0, top_sampling=False,
                     random_sampling=False, context=None, cache=None, ngram=None, memory=None):
        """``memory`` (keyword): a :class:`jlm_amd.memory.MemoryMix` of this model -- the mass of the k nearest entries of every
        hypothesis's state in a memory of (hidden state, next word) pairs is mixed into every edge cost, p = (1 - lam) p_lm + lam c_r
        (DESIGN.md section 30), with or without ``context``; lam = 0 is the decode without.  ValueError with ``cache=`` / a
        CachedContext, ``ngram=``, ``vocab_select`` or ``compat_quirks``, for a memory of another model, and for a device batch of more
        than 65 535 rows (``max_batch`` x beam), before anything runs.
        ``ngram`` (keyword): a :class:`jlm_amd.ngram.NGramMix` -- a back-off word n-gram model is mixed into every edge cost,
        p = (1 - lam) p_lm + lam p_ng(w | the last words of [<eos>] + context + the path so far), with or without
        ``context``.  ValueError with ``cache=`` / a CachedContext, ``vocab_select`` or ``compat_quirks``, for anything that is not an
        NGramMix and for a table with a word id outside the model's vocabulary, before anything runs.
        ``cache`` (keyword): a :class:`jlm_amd.cache.CacheSpec` (one theta, N <= 4096) beside ``context`` word lists, or a
        :class:`jlm_amd.context.CachedContext` as ``context`` (``self.model.prime(contexts, cache=...)``): the continuous cache over
        every input's own context -- its last N (state, next word) pairs -- is mixed into every edge cost, p = (1 - lam) p_lm + lam c
        (DESIGN.md section 21); an input without context words is decoded as without a cache, and so is lam = 0.  ValueError with
        ``vocab_select`` or ``compat_quirks``, before anything runs.
        ``context`` (keyword): the words committed in front of every input -- a list with one entry per input (None, empty, or a
        sequence of word ids / lexicon strings; a string outside the vocabulary reads as <unk>), or a ContextState of one row per input
        (``self.model.prime``), which any number of calls may reuse.  Input i is decoded as the continuation of
        [<eos>] + context[i] (jlm_amd/context.py); scores are -log p(path | that history).  None, or nothing but empty entries: the
        reference's decode."""
        inputs = list(inputs)
        if memory is not None:
            memory = self._check_memory(memory, context, cache, ngram, vocab_select)
        if ngram is not None:
            self._check_ngram(ngram, context, cache, vocab_select)
        mix_kw = dict(ngram=ngram) if ngram is not None else (dict(memory=memory) if memory is not None else {})
        if memory is not None and beam_width is not None and 1 <= int(beam_width) <= self.MAX_BEAM:
            # (the retrieval addresses a batch's rows through 16 bits; before the context is resolved, as every refusal)
            n_sent = max((len(c) for c in self._chunks(inputs, int(beam_width))), default=0)
            if n_sent * int(beam_width) > 65535:
                raise ValueError("a decode under a memory takes at most 65535 rows a device batch (%d sentences x beam %d): lower "
                                 "Decoder.max_batch" % (n_sent, int(beam_width)))
        if vocab_select:                     # (before the context is resolved: nothing is primed for a call that is refused)
            self._refuse_cache(context, "vocab_select", cache)
        if self.compat_quirks:
            self._refuse_cache(context, "compat_quirks", cache)
        ctx = self._context(context, len(inputs), cache=cache)
        sel = (vocab_select, samples, top_sampling, random_sampling)
        if beam_width is None:       # the reference's unpruned search, sentence at a time on the host
            host_mem = self._host_memory(memory)              # (the memory is read back once a call)
            return [self._search_on_host(x, self._host_context(ctx, i), topN, None, *sel, **self._host_ngram(ngram, ctx, i), **host_mem)
                    for i, x in enumerate(inputs)]
        if not 1 <= int(beam_width) <= self.MAX_BEAM:
            raise ValueError("beam_width must be 1..%d on the GPU path (or None: the unpruned host-side search)" % self.MAX_BEAM)
        if not inputs:
            return []
        if self.compat_quirks and not vocab_select and self.lattice_vocab:
            # decoder.py:176: `if self.lattice_vocab:` is still true after an earlier vocab_select call, so the full-vocabulary
            # call indexes the OLD list: ValueError for a word outside it, else the old list is what the rows are normalised over
            if ctx is not None:
                raise ValueError("compat_quirks: the stale-vocabulary path of the reference takes no left context")
            return [self._decode_stale_vocab(x, topN, beam_width) for x in inputs]
        if not all(inputs):        # (an empty string / list is falsy)
            return self._decode_subset(inputs, [i for i, x in enumerate(inputs) if len(x)], ctx, topN, beam_width, *sel, **mix_kw)
        chunks = self._chunks(inputs, beam_width, reorder=not (samples and random_sampling))
        workers = 1 if (samples and random_sampling) else self.prefetch_workers
        extra, engine_kw, left = None, lambda _none: dict(vocab=None, **mix_kw), None
        if vocab_select:
            # a chunk's word lists beside its lattice: (words, off) the engine's CSR over its sentences, lists[k] sentence k's own
            extra = lambda idx, lat: lat.static_vocab(samples, top_sampling, random_sampling, len(self.w2i))
            engine_kw = lambda vocab: dict(vocab=vocab[:2])

            def left(vocab, k):      # the reference leaves the LAST sentence's list behind
                self.lattice_vocab = vocab[2][k]
        try:
            out = self._launch_chunks(self._prepare_chunks(inputs, chunks, beam_width, workers, extra), chunks, len(inputs), ctx, topN,
                                      beam_width, "static", engine_kw, left)
        except _CellTooLarge as e:
            return self._heavy_on_host(e.sentences, inputs, ctx, topN, beam_width, *sel, **mix_kw)
        self.perf_sen += len(inputs)
        return out

    def _decode_subset(self, inputs, keep, ctx, *args, ngram=None, memory=None):
        """decode_batch(*args) of the inputs ``keep`` alone, their context rows with them -> the whole call's result list: theirs in place,
        [(0.0, [])] everywhere else -- an empty input's: the reference's loop leaves the <eos> path alone (decoder.py:220-241)"""
        sub = self.decode_batch([inputs[i] for i in keep], *args, context=ctx.sub(keep) if ctx is not None else None,
                                **(dict(ngram=ngram) if ngram is not None else {}),
                                **(dict(memory=memory) if memory is not None else {})) if keep else []
        out = [[(0.0, [])] for _ in inputs]
        for i, r in zip(keep, sub):
            out[i] = r
        return out

    def _heavy_on_host(self, heavy, inputs, ctx, *args, ngram=None, memory=None):
        """The rest of a decode_batch(*args) call that met _CellTooLarge: the sentences named take the host-side search with the beam
        (_search_on_host), everything else goes through the device again -> the call's result list."""
        heavy = set(heavy)
        out = self._decode_subset(inputs, [i for i in range(len(inputs)) if i not in heavy], ctx, *args,
                                  **(dict(ngram=ngram) if ngram is not None else {}), **(dict(memory=memory) if memory is not None else {}))
        lv_last = self.lattice_vocab
        host_mem = self._host_memory(memory)
        for i in sorted(heavy):
            out[i] = self._search_on_host(inputs[i], self._host_context(ctx, i), *args, **self._host_ngram(ngram, ctx, i), **host_mem)
        if (len(inputs) - 1) not in heavy:
            self.lattice_vocab = lv_last      # (the reference leaves the LAST sentence's list behind)
        return out

    # The chunk pipeline under decode_batch, decode_predict_batch and DynamicDecoder.decode_batch: _prepare_chunks is its host side,
    # _launch_chunks its device side (decode_predict_batch drains the first before it starts the second).  What the three differ in comes
    # as values: ``extra(idx, lat)``, what a chunk needs beside its lattice (word lists, spans), ``engine_kw(that)``, the engine's
    # keywords made of it, and ``left(that, k)``, called when the chunk that holds the call's last input -- at position k -- is submitted.
    def _prepare_chunks(self, texts, chunks, beam_width, workers, extra=None):
        """Every chunk's _Chunk, in order and up to ``workers`` + 1 ahead of the consumer (_prefetched): the lattice (native, releases the
        GIL), the check of its cells (_CellTooLarge) and ``extra``'s addition (None: none)."""
        def prepare(idx):
            lat = BatchLattice(self._builder, [texts[j] for j in idx], beam_width, pool=self._engine.staging_pool)
            self._check_cells(lat, idx, beam_width)
            return _Chunk(idx, lat, extra(idx, lat) if extra is not None else None)
        return self._prefetched(prepare, chunks, workers)

    def _launch_chunks(self, prepared, chunks, n, ctx, topN, beam_width, kind, engine_kw, left=None):
        """The prepared chunks of a call of n inputs through the device pipeline (_run_pipeline): each is submitted with its rows of
        ``ctx``, collected in order and scattered -> the call's result list."""
        out = [None] * n

        def submit(ch):
            self.last_lattice = ch.lat
            if left is not None and (n - 1) in ch.idx:
                left(ch.extra, ch.idx.index(n - 1))
            return ch.idx, self._engine.submit(ch.lat, kind, topN=topN, timing=self.perf_timing,
                                               context=ctx.for_chunk(ch.idx) if ctx is not None else None, **engine_kw(ch.extra))

        def finish(idx, ticket):
            for j, r in zip(idx, self._engine.collect(ticket)):
                out[j] = r
            if ticket.lat is not self.last_lattice:        # (the lattice the caller may still look at keeps its arrays)
                ticket.lat.release()
            self._log_perf()

        self._run_pipeline(prepared, len(chunks), submit, finish, depth=self.depth_for(max(len(c) for c in chunks), beam_width))
        return out

    @staticmethod
    def _host_context(ctx, i):
        """what a host-side search takes of input i's left context: None or a jlm_amd.context.HostContext"""
        return ctx.host(i) if ctx is not None else None

    @staticmethod
    def _host_ngram(ngram, ctx, i):
        """the keywords a host-side search takes of the call's ``ngram=`` for input i: none, or ngram = (the NGramMix, the last words of
        the input's history [<eos>] + context)"""
        if ngram is None:
            return {}
        from .generate import EOS_ID
        return dict(ngram=(ngram, ctx.tail(i) if ctx is not None else [EOS_ID]))

    @staticmethod
    def _host_memory(memory):
        """the keywords a host-side search takes of the call's ``memory=``: none, or memory = mix(pred [rows, V], h [rows, H]) ->
        (1 - lam) pred + lam c(h), the float64 definition over the memory read back once (memory.memory_distribution)"""
        if memory is None:
            return {}
        import numpy as np
        from .memory import memory_distribution
        keys, words = memory.memory.numpy()
        keys = keys.astype(np.float64)

        def mix(pred, h):
            pred = np.array(pred, dtype=np.float64)
            for q in range(pred.shape[0]):
                pred[q] = (1.0 - memory.lam) * pred[q] + memory.lam * memory_distribution(h[q], keys, words, memory.theta, memory.k, pred.shape[1])
            return pred
        return dict(memory=mix)

    def _search_on_host(self, input, context, topN, beam_width, vocab_select, samples, top_sampling, random_sampling, ngram=None,
                        memory=None):
        """one input searched on the host over LSTM_Model's numpy API: every input of a call with beam_width=None, and with the beam a
        sentence whose lattice cells the device beam step cannot hold"""
        return self._decode_unpruned(input, topN, vocab_select, samples, top_sampling, random_sampling, beam_width=beam_width,
                                     context=context, ngram=ngram, memory=memory)

    def _cand_limit(self, lat, beam_width):
        """candidates of one lattice cell the device beam step accepts for this batch shape"""
        if self.CAND_LIMIT is not None:
            return int(self.CAND_LIMIT)
        from . import ops
        mode = 2 if self.dynamic else (1 if self.model.dev.self_norm else 0)
        frames = (lat.n_frames + 7) // 8 * 8                       # as the plans round it (engine._plan_for)
        return int(ops.backend().beam_step_max_cands(int(beam_width), frames, mode))

    def _check_cells(self, lat, idx, beam_width):
        if lat.n_sent == 0:
            return
        limit = self._cand_limit(lat, beam_width)
        if lat.max_cands <= limit:
            return
        import numpy as np
        per_sentence = np.diff(np.asarray(lat.end_off)).reshape(lat.n_frames, lat.n_sent).max(axis=0)
        raise _CellTooLarge([idx[k] for k in range(lat.n_sent) if int(per_sentence[k]) * beam_width > limit])

    def depth_for(self, n_sent, beam_width):
        """Chunks in flight for chunks of n_sent sentences: four (one per stream) while a chunk's frame is a few thousand rows and its
        kernels leave room for the others', three above 8 192 rows (BASELINE configs[2]: 1 024 sentences x beam 20 -- 41.8 vs 43.4 ms
        per step; the vocabulary kernel alone takes 1.8 ms there and a fourth batch only adds to the queue)."""
        return min(self.pipeline_depth, 3) if int(n_sent) * int(beam_width or 1) > 8192 else self.pipeline_depth

    def _run_pipeline(self, prepared, n_chunks, submit, finish, depth=None):
        """The device pipeline of decode_batch: ``submit`` every prepared chunk (enqueue upload + frame loop + read-back: no
        waiting), ``finish`` them in order (wait for the batch, build its n-best lists).  ``pipeline_depth`` + 1 chunks are in
        flight at most (the engine alternates streams; a chunk owns its plan's buffers until finished).
"""
        # The n-best lists are ~8 k acyclic containers per 256-sentence chunk: left on, the cyclic collector runs a dozen
        # young collections per chunk and, as the result list grows, full collections over everything decoded so far (4.0 vs
        # 2.9 ms per chunk at 200 vs 40 chunks per call).  Nothing allocated in here can form a cycle: collection is paused.
        gc_was_on = gc.isenabled()
        pause_gc = gc_was_on and os.environ.get("JLM_NO_GC_PAUSE", "0") != "1"
        if pause_gc:
            gc.disable()
        self._engine.pipelined = n_chunks > 1          # more than one batch in flight: the vocabulary kernel leaves CUs to the others
        try:
            self._run_pipeline_nogc(prepared, n_chunks, submit, finish, depth or self.pipeline_depth)
        finally:
            self._engine.pipelined = False
            if pause_gc:
                gc.enable()

    def _run_pipeline_nogc(self, prepared, n_chunks, submit, finish, depth):
        inflight = deque()
        try:
            for item in prepared:
                inflight.append(submit(item))
                if len(inflight) > depth:
                    finish(*inflight.popleft())
            while inflight:
                finish(*inflight.popleft())
        except BaseException:
            while inflight:                      # chunks already on the device: wait for them, their plans are released
                _idx, ticket = inflight.popleft()
                try:
                    self._engine.collect(ticket)
                except Exception:
                    pass
            raise

    def _chunks(self, inputs, beam_width, reorder=True):
        """Index lists of the device batches of one decode_batch call.  A batch's frame loop and buffers run to its LONGEST
        sentence (frames x sentences x beam state rows of 2 H + ldt floats: every frame's state stays resident, a lattice word
        may reach back any number of frames), so sentences are dealt by decreasing length -- as shard.py deals them over the
        ranks -- and a batch closes at ``max_batch`` sentences or when its state rows would exceed ``plan_budget_bytes``: one
        200-kana input costs its own small batch, not 12 GB for the 1 023 short sentences that happened to follow it.
        reorder=False keeps the caller's order (random_sampling draws from the global RNG sentence by sentence)."""
        import numpy as np
        n = len(inputs)
        m = self.model.dev
        row_bytes = (2 * m.H + (m.ldt if (m.mode != "untied" or m.split_lstm) else 0)) * 4 + 64
        fits = lambda longest: max(1, min(self.max_batch, self.plan_budget_bytes // (((longest + 1 + 7) // 8 * 8) * beam_width * row_bytes)))
        lens = np.fromiter(map(len, inputs), dtype=np.int64, count=n)
        if reorder and n > self.max_batch:
            # longest first: a chunk's frame count is its FIRST sentence's, so its size is one division -- no per-sentence
            # Python work (a 10 240-sentence call spent 9 ms here, before the first launch, as a loop)
            order = np.argsort(-lens, kind="stable")
            chunks, i = [], 0
            while i < n:
                k = fits(int(lens[order[i]]))
                chunks.append(order[i:i + k].tolist())
                i += k
            return chunks
        chunks, cur, longest = [], [], 0
        for i in range(n):
            li = int(lens[i])
            if cur and len(cur) >= fits(max(longest, li)):
                chunks.append(cur)
                cur, longest = [], 0
            cur.append(i)
            longest = max(longest, li)
        if cur:
            chunks.append(cur)
        return chunks

    def _decode_unpruned(self, input, topN, vocab_select, samples, top_sampling, random_sampling, beam_width=None, vocab=None,
                         context=None, ngram=None, memory=None):
        """Decoder.decode of the reference with ``beam_width=None`` (decoder.py:220-241), statement for statement on the
        host: every candidate survives, each frame is one ``predict_with_context`` call over all of its paths (the GPU
        kernels behind LSTM_Model's numpy API), the result is the final frame in generation order, unsorted.  Also the
        engine of :meth:`_decode_stale_vocab` (a beam and a fixed vocabulary list).  ``context``: None, or a context.HostContext: h, c
        [1, H] -- the primed state read back -- and word, the last of the history: what the root consumes, and from where; mix(pred, h)
        under the continuous cache: every frame's probabilities become the mixture (context.DecodeContext.host_mixer).  ``ngram``: None,
        or (an NGramMix, the last words of the history): every path keeps its last two words and its probabilities become the n-gram
        mixture by the float64 definition (jlm_amd/ngram.py).  ``memory``: None, or mix(pred, h) of a memory
        (:meth:`_host_memory`): the same plug as the cache's, on every frame of every input."""
        import math
        import numpy as np
        if len(input) == 0:
            return [(0.0, [])]
        lat = self.last_lattice = BatchLattice(self._builder, [input], 1)
        ends = lat.backward_lookup(0)
        if vocab is None and vocab_select:
            vocab = list(lat.static_vocab(samples, top_sampling, random_sampling, len(self.w2i))[2][0])
            self.lattice_vocab = vocab
        col = (lambda w: vocab.index(w)) if vocab is not None else (lambda w: w)       # ValueError for a word outside the list
        H = self.model.hidden_size
        # a path: (score, nodes tuple, word id of its last node); per frame also its state rows and probability rows
        frames = {0: dict(paths=[(0.0, (), ends[0][0][2] if context is None else int(context.word))])}
        if ngram is not None:
            assert vocab is None
            frames[0]["hist"] = [tuple(ngram[1])[-2:]]
            q_of = {}                                        # history -> exp q(. | history) over the vocabulary
        for i in range(len(input) + 1):
            if i > 0:
                paths = []
                for (st, _ln, w, word) in ends[i]:
                    prev = frames[st if st >= 0 else 0]
                    c = col(w)
                    for k, (score, nodes, _lw) in enumerate(prev["paths"]):
                        paths.append((score - math.log(prev["pred"][k][c]), nodes + (word,), w, st if st >= 0 else 0, k))
                if beam_width is not None:
                    paths.sort(key=lambda x: x[0])          # stable, like list.sort in the reference
                    paths = paths[:beam_width]
                if len(paths) > self.max_unpruned_paths:
                    raise ValueError("beam_width=None: frame %d holds %d hypotheses (max_unpruned_paths = %d)" % (
                        i, len(paths), self.max_unpruned_paths))
                frames[i] = dict(paths=[(p[0], p[1], p[2]) for p in paths], src=[(p[3], p[4]) for p in paths])
                if ngram is not None:
                    frames[i]["hist"] = [(frames[p[3]]["hist"][p[4]] + (int(p[2]),))[-2:] for p in paths]
            cur = frames[i]
            if i == len(input):
                break                                        # (the reference steps the last frame too and drops the result)
            if i == 0:
                hid, cel = (np.zeros((1, H)), np.zeros((1, H))) if context is None else (np.asarray(context.h), np.asarray(context.c))
            else:
                hid = np.stack([frames[f]["h"][k] for f, k in cur["src"]])
                cel = np.stack([frames[f]["c"][k] for f, k in cur["src"]])
            if not cur["paths"]:
                cur["pred"], cur["h"], cur["c"] = [], [], []
                continue
            (pred, _y, _t1, _t2), h2, c2 = self.model.predict_with_context([p[2] for p in cur["paths"]], hid, cel, vocab)
            if context is not None and context.mix is not None:
                pred = context.mix(pred, h2)
            if memory is not None:
                assert vocab is None
                pred = memory(pred, h2)
            if ngram is not None:
                pred = np.array(pred, dtype=np.float64)
                for k, hk in enumerate(cur["hist"]):
                    if hk not in q_of:
                        q_of[hk] = np.exp(ngram[0].table.logq_all(hk, pred.shape[1]))
                    pred[k] = (1.0 - ngram[0].lam) * pred[k] + ngram[0].lam * q_of[hk]
            cur["pred"], cur["h"], cur["c"] = pred, h2, c2
        out = [(score, [w for w in nodes if w != "<eos>"]) for score, nodes, _lw in frames[len(input)]["paths"]]
        self.perf_sen += 1
        return out[:topN]

    def _decode_stale_vocab(self, input, topN, beam_width):
        """compat_quirks: a full-vocabulary call after a vocab_select call keeps normalising over the old list
        (decoder.py:62,176) -- ValueError from ``list.index`` when the lattice has a word outside it."""
        return self._decode_unpruned(input, topN, False, 0, False, False, beam_width=beam_width, vocab=list(self.lattice_vocab))

    def _prefetched(self, prepare, starts, workers=1):
        """prepare(start) for every chunk, results in order, up to ``workers`` + 1 chunks ahead of the consumer:
        with more than one chunk the lattices are built on worker threads (the native builder releases the GIL)
        while this thread enqueues launches and builds strings.  workers=1 keeps the calls themselves in
        order (needed when prepare draws from the global RNG: random_sampling)."""
        starts = list(starts)
        if len(starts) <= 1:
            for i in starts:
                yield prepare(i)
            return
        from concurrent.futures import ThreadPoolExecutor
        workers = max(1, min(workers, self.prefetch_workers))
        # the workers pin themselves to the CPUs of their GPU's NUMA node when they start (jlm_amd/numa.py; the thread only)
        from . import numa
        if getattr(self, "_numa", None) is None:
            dev = getattr(self.model, "device", None)
            idx = dev.index if (dev is not None and dev.type == "cuda" and dev.index is not None) else 0
            self._numa = (numa.worker_cpus(idx, min_cpus=max(numa.MIN_PIN_CPUS, self.prefetch_workers + 1))
                          if (dev is not None and dev.type == "cuda") else (-1, set()))
        pin = (lambda cpus=self._numa[1]: numa.pin_current_thread(cpus))
        if workers == 1:
            if self._pool1 is None:          # a pool of ONE thread runs its tasks in submission order
                self._pool1 = ThreadPoolExecutor(max_workers=1, thread_name_prefix="jlm-lattice", initializer=pin)
            pool = self._pool1
        else:
            if self._pool is None:
                self._pool = ThreadPoolExecutor(max_workers=self.prefetch_workers, thread_name_prefix="jlm-lattice", initializer=pin)
            pool = self._pool
        ahead = workers + 1
        submit = lambda i: pool.submit(prepare, i)
        futs = deque(submit(i) for i in starts[:ahead])
        for j in range(len(starts)):
            item = futs.popleft().result()
            if j + ahead < len(starts):
                futs.append(submit(starts[j + ahead]))
            yield item

    def decode(self, input, topN=10, beam_width=10, vocab_select=False, samples=0, top_sampling=False,
               random_sampling=False, context=None, cache=None, ngram=None, memory=None):
        """``context`` (keyword): the words committed in front of ``input`` -- one sequence of word ids / lexicon strings, or a
        ContextState of one row (see decode_batch); ``cache``, ``ngram``, ``memory``: decode_batch's."""
        out = self.decode_batch([input], topN, beam_width, vocab_select, samples, top_sampling, random_sampling,
                                context=_Single(context), cache=cache, **(dict(ngram=ngram) if ngram is not None else {}),
                                **(dict(memory=memory) if memory is not None else {}))[0]
        if len(input):
            # the reference's shape: dict frame -> [Node] (decoder.py:79-135), what _build_lattice returns
            self.backward_lookup = {f: [Node(st, ln, w, word) for (st, ln, w, word) in nodes]
                                    for f, nodes in enumerate(self.last_lattice.backward_lookup(0))}
        return out


    # ------------------------------------------------------------------ conversion of an unfinished reading
    MAX_PREDICTIONS = 64         # jlm_tail_predict's n_out: one thread per rank
    _EMPTY_INPUT = "ア"      # an empty input is decoded as this one kana for the sake of its frame 0: the root's distribution

    def _tail_spans(self, text, index):
        """the tail starts of one input: [(s, lo, hi)] for every s in [0, len) at which vocabulary words properly extend text[s:]"""
        return index.tail_spans(text if isinstance(text, str) else "".join(text))

    def decode_predict_batch(self, inputs, topN=10, beam_width=10, context=None, cache=None, ngram=None, memory=None):
        """Conversion while the user types: every input is kana whose LAST word may be unfinished.  -> per input a pair
        (conversions, predictions).  ``conversions`` is ``decode_batch(inputs, topN, beam_width, context=context)``'s list, the very
        launches and bits.  ``predictions`` is [(score, [word, ...])], at most ``topN`` (1 .. 64), ascending: the best paths that cover
        input[:s] with lattice words -- a hypothesis the beam kept at frame s -- and end in one vocabulary word whose reading starts with
        input[s:] and is longer, over every such s; score = the hypothesis's score - log p(word | it) under the full vocabulary.  Ties
        keep (s, the word's (reading, id) order, the hypothesis's rank).  The two lists are not merged: a path with one word fewer scores
        better.  An empty input gives ([(0.0, [])], the likeliest words that have a reading at all).  One more launch per batch behind
        the frame loop (jlm_tail_predict); only (frame, lo, hi) triples travel per sentence, never word lists.
        ValueError before any launch: ``beam_width=None``, ``topN`` outside 1 .. 64, compat_quirks with a stale vocabulary, a sentence
        with a lattice cell the device beam step cannot hold.  TypeError for the other decoders: their rows are not normalised over the
        full vocabulary, or are not words."""
        if self.dynamic or self.char_model:
            raise TypeError("%s has no decode_predict: the last word is predicted from rows normalised over the full word vocabulary "
                            "(the static Decoder)" % type(self).__name__)
        inputs = list(inputs)
        if memory is not None:
            raise ValueError("decode_predict takes no memory (DESIGN.md section 30: Decoder.decode only)")
        if ngram is not None:
            raise ValueError("decode_predict takes no n-gram mixture (DESIGN.md section 24: Decoder.decode only)")
        if cache is not None:
            raise ValueError("decode_predict takes no continuous cache (DESIGN.md section 21: Decoder.decode only)")
        self._refuse_cache(context, "decode_predict")
        if beam_width is None:
            raise ValueError("decode_predict needs a beam (beam_width=None is the unpruned host-side search)")
        if not 1 <= int(beam_width) <= self.MAX_BEAM:
            raise ValueError("beam_width must be 1..%d" % self.MAX_BEAM)
        if isinstance(topN, bool) or int(topN) != topN or not 1 <= int(topN) <= self.MAX_PREDICTIONS:
            raise ValueError("topN must be an integer in 1..%d (got %r)" % (self.MAX_PREDICTIONS, topN))
        topN, beam_width = int(topN), int(beam_width)
        if self.compat_quirks and self.lattice_vocab:
            raise ValueError("compat_quirks: the stale-vocabulary path of the reference normalises over an old word list; predictions need "
                             "the full vocabulary")
        if not inputs:
            return []
        import numpy as np
        index = self.model.reading_index()
        # the batches of decode_batch over the inputs that have kana (the same chunks: the same bits), then the empty inputs as one more
        full = [i for i, x in enumerate(inputs) if len(x)]
        empty = [i for i, x in enumerate(inputs) if not len(x)]
        texts = [x if len(x) else self._EMPTY_INPUT for x in inputs]
        sub = [inputs[i] for i in full]
        chunks = [[full[j] for j in c] for c in self._chunks(sub, beam_width)] if full else []
        for a in range(0, len(empty), self.max_batch):
            chunks.append(empty[a:a + self.max_batch])

        def spans(idx, _lat):
            """the chunk's tail spans in CSR, as the engine takes them: (off [len(idx) + 1], frame, lo, hi)"""
            spans = [self._tail_spans(inputs[j], index) if len(inputs[j]) else [(0,) + tuple(index.ranges(""))[1:]] for j in idx]
            off = np.zeros(len(idx) + 1, dtype=np.int32)
            np.cumsum([len(s) for s in spans], out=off[1:])
            flat = np.array([t for s in spans for t in s], dtype=np.int32).reshape(-1, 3)
            return off, flat[:, 0].copy(), flat[:, 1].copy(), flat[:, 2].copy()

        # every lattice before the first launch (the priming of the contexts included): a refusal leaves nothing enqueued
        prepared = []
        try:
            for chunk in self._prepare_chunks(texts, chunks, beam_width, self.prefetch_workers, spans):
                prepared.append(chunk)
        except _CellTooLarge as e:
            for chunk in prepared:
                chunk.lat.release()
            raise ValueError("decode_predict: input(s) %s have a lattice cell with more candidates than the device beam step holds at "
                             "beam %d (decode_batch would search them on the host); convert them with decode" %
                             (", ".join("%d (%r)" % (i, inputs[i]) for i in sorted(e.sentences)), beam_width))
        ctx = self._context(context, len(inputs))
        if getattr(self, "_predict_ids", None) is None:
            import torch
            self._predict_ids = torch.from_numpy(np.ascontiguousarray(index.ids, dtype=np.int32)).to(self.model.dev.device)
        out = self._launch_chunks(iter(prepared), chunks, len(inputs), ctx, topN, beam_width, "static",
                                  lambda sp: dict(predict=(sp, self._predict_ids, self.i2w, topN)))
        for j in empty:
            out[j] = ([(0.0, [])], out[j][1])
        self.perf_sen += len(full)
        return out

    def decode_predict(self, input, topN=10, beam_width=10, context=None, cache=None, ngram=None, memory=None):
        """:meth:`decode_predict_batch` of one input -> (conversions, predictions); ``context`` as :meth:`decode` takes it."""
        if self.dynamic or self.char_model:
            raise TypeError("%s has no decode_predict (see Decoder.decode_predict_batch)" % type(self).__name__)
        out = self.decode_predict_batch([input], topN, beam_width, context=_Single(context), cache=cache, ngram=ngram, memory=memory)[0]
        if len(input):
            self.backward_lookup = {f: [Node(st, ln, w, word) for (st, ln, w, word) in nodes]
                                    for f, nodes in enumerate(self.last_lattice.backward_lookup(0))}
        return out


    # ------------------------------------------------------------------ per-segment candidate lists
    MAX_CANDIDATES = 64

    def decode_candidates_batch(self, inputs, topN=10, beam_width=10, n_cand=10, lookahead=None, rank=0, context=None, memory=None):
        """The window an input method shows: per input a pair (conversions, segments).  ``conversions`` is
        ``decode_batch(inputs, topN, beam_width, context=context)``'s list, the very chunks, launches and bits.  ``segments`` cuts
        path ``rank`` of it into its words: [(start, length, [(score, word), ...]), ...] in path order, where a segment's list holds the
        lattice words with that start and length -- the path's own and the raw-kana fallback among them --, at most ``n_cand``
        (1 .. 64), ascending by (score, lattice node order).  score = -log p of the path with the segment's word replaced: the
        hypothesis's score in front of the segment - log p(word | it), then the next ``lookahead`` words of the path re-scored behind
        the substitute under the full vocabulary (None: all of them), then the path's own terms for the rest; the path's own word
        scores what the path scores, up to rounding.  An empty input gives ([(0.0, [])], []), an input with fewer than rank + 1
        paths gives segments = [].  Per chunk one more op behind the collected decode (``torch.ops.jlm.alt_frames``); the plan stays
        busy until its lists are read.
        ValueError before any launch, every lattice built first: ``beam_width=None``, ``n_cand`` outside 1 .. 64, a negative
        ``lookahead`` or ``rank``, ``rank >= topN``, compat_quirks with a stale vocabulary, a sentence with a lattice cell the device
        beam step cannot hold, a CachedContext.  TypeError for the other decoders: their rows are not normalised over the full
        vocabulary, or are not words."""
        if self.dynamic or self.char_model:
            raise TypeError("%s has no decode_candidates: a segment's alternatives are scored on rows normalised over the full word "
                            "vocabulary (the static Decoder)" % type(self).__name__)
        inputs = list(inputs)
        if memory is not None:
            raise ValueError("decode_candidates takes no memory (DESIGN.md section 30: Decoder.decode only)")
        self._refuse_cache(context, "decode_candidates")
        from .context import CachedContext, DecodeContext
        state = context.context if isinstance(context, _Single) else context
        state = state.state if isinstance(state, DecodeContext) else state
        if isinstance(state, CachedContext):
            raise ValueError("decode_candidates takes no CachedContext (DESIGN.md section 25: the cache rewrites edge costs per hypothesis)")
        if beam_width is None:
            raise ValueError("decode_candidates needs a beam (beam_width=None is the unpruned host-side search)")
        if not 1 <= int(beam_width) <= self.MAX_BEAM:
            raise ValueError("beam_width must be 1..%d" % self.MAX_BEAM)
        is_int = lambda x: not isinstance(x, bool) and int(x) == x
        if not is_int(n_cand) or not 1 <= int(n_cand) <= self.MAX_CANDIDATES:
            raise ValueError("n_cand must be an integer in 1..%d (got %r)" % (self.MAX_CANDIDATES, n_cand))
        if lookahead is not None and (not is_int(lookahead) or int(lookahead) < 0):
            raise ValueError("lookahead must be None or an integer >= 0 (got %r)" % (lookahead,))
        if not is_int(topN) or not is_int(rank) or not 0 <= int(rank) < int(topN):
            raise ValueError("rank must be an integer in 0..topN - 1 (got rank %r, topN %r)" % (rank, topN))
        topN, beam_width, n_cand, rank = int(topN), int(beam_width), int(n_cand), int(rank)
        lookahead = None if lookahead is None else int(lookahead)
        if self.compat_quirks and self.lattice_vocab:
            raise ValueError("compat_quirks: the stale-vocabulary path of the reference normalises over an old word list; candidates need "
                             "the full vocabulary")
        if not inputs:
            return []
        # the batches of decode_batch over the inputs that have kana: the same chunks, the same bits
        full = [i for i, x in enumerate(inputs) if len(x)]
        out = [([(0.0, [])], []) for _ in inputs]
        if not full:
            return out
        chunks = [[full[j] for j in c] for c in self._chunks([inputs[i] for i in full], beam_width)]
        # every lattice before the first launch (the priming of the contexts included): a refusal leaves nothing enqueued
        prepared = []
        try:
            for chunk in self._prepare_chunks(inputs, chunks, beam_width, self.prefetch_workers):
                prepared.append(chunk)
        except _CellTooLarge as e:
            for chunk in prepared:
                chunk.lat.release()
            raise ValueError("decode_candidates: input(s) %s have a lattice cell with more candidates than the device beam step holds at "
                             "beam %d (decode_batch would search them on the host); convert them with decode" %
                             (", ".join("%d (%r)" % (i, inputs[i]) for i in sorted(e.sentences)), beam_width))
        ctx = self._context(context, len(inputs))
        eng = self._engine

        def submit(ch):
            self.last_lattice = ch.lat
            return ch.idx, eng.submit(ch.lat, "static", topN=topN, timing=self.perf_timing,
                                      context=ctx.for_chunk(ch.idx) if ctx is not None else None, vocab=None)

        def finish(idx, ticket):
            conv = eng.collect(ticket, keep=True)            # phase 1; the plan's pools are read once more
            try:
                segs = eng.candidates(ticket, rank, lookahead, n_cand)
            finally:
                ticket.plan.busy = False
            for j, c, sg in zip(idx, conv, segs):
                out[j] = (c, sg)
            if ticket.lat is not self.last_lattice:
                ticket.lat.release()
            self._log_perf()

        # (phase 2 is not pipelined across chunks: a chunk is finished before the next is submitted)
        eng.pipelined = len(chunks) > 1                      # (as decode_batch sets it for the call's chunks)
        done = 0
        try:
            for ch in prepared:
                done += 1
                finish(*submit(ch))
        finally:
            eng.pipelined = False
            for ch in prepared[done:]:                       # a failure: the chunks never submitted give their blocks back
                ch.lat.release()
        self.perf_sen += len(full)
        return out

    def decode_candidates(self, input, topN=10, beam_width=10, n_cand=10, lookahead=None, rank=0, context=None, memory=None):
        """:meth:`decode_candidates_batch` of one input -> (conversions, segments); ``context`` as :meth:`decode` takes it."""
        if self.dynamic or self.char_model:
            raise TypeError("%s has no decode_candidates (see Decoder.decode_candidates_batch)" % type(self).__name__)
        out = self.decode_candidates_batch([input], topN, beam_width, n_cand, lookahead, rank, context=_Single(context), memory=memory)[0]
        if len(input):
            self.backward_lookup = {f: [Node(st, ln, w, word) for (st, ln, w, word) in nodes]
                                    for f, nodes in enumerate(self.last_lattice.backward_lookup(0))}
        return out


class _Single:
    """the ``context=`` of a one-input call on its way through the batch method: resolved there, after the argument checks"""

    def __init__(self, context):
        self.context = context


def __getattr__(name):
    """``from decoder import Decoder, CharRNNDecoder`` (reference decoder/eval.py:7): the character-model decoder lives in
    jlm_amd/decoder_char.py (which imports this module), resolved on first use"""
    if name == "CharRNNDecoder":
        from .decoder_char import CharRNNDecoder
        return CharRNNDecoder
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
