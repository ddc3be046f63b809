"""Frame-synchronous batched lattice decode on one MI355X.

All sentences of a batch advance one kana frame at a time; every frame is a
fixed sequence of kernel launches with no host synchronisation until the
n-best read-out:

  static (Decoder.decode, reference decoder.py:220-241), frame f:
    beam_step(f)                     K7+K8  candidates, stable top-k, back pointers
    lstm_step(live rows of f)        K1+K2+K3+K9 fused gate GEMM
    project_T                        K4 (+ V_table projections)
    full_vocab_lse | wordlist_lse    K5+K6 fused log-normaliser (never the logits)
    edge_logits(nodes starting at f) logits the lattice can consume next
                                     (side stream: independent of the normaliser)

  dynamic (DynamicDecoder.decode, reference decoder_dynamic.py:177-194), frame f:
    wordlist_lse(merge) on frames <= f-2 with the words new at f   (K11)
    beam_step(f, mode 2)             re-scores every path from the head (K12)
    lstm_step / project_T / wordlist_lse(init list of f) / edge_logits

The reference evaluates frame i-1 lazily at step i (decoder_dynamic.py:130);
stepping it eagerly is the same arithmetic.  The final frame is never stepped
(decoder_dynamic.py never does; decoder.py does and discards the result).

Buffers live in per-shape plans that are reused across batches (no allocation or
re-upload of constants per batch).  submit()/collect() split a decode into the
asynchronous device part and the host read-out, so the strings of batch i are
built while the GPU decodes batch i+1 (two plans of the same shape alternate).

Upload, the whole launch sequence and the read-back of a batch are ONE custom op (torch.ops.jlm.decode_batch ->
jlm_decode_frames, csrc/jlm_decode.hip): no host work between the frames, none of it under the interpreter lock.
"""
import os
import threading
from collections import namedtuple

import numpy as np

from . import _lib
from . import ops

# what DecodeEngine.submit returns for collect: the batch's plan (its buffers until collected) and lattice, topN and timing as submitted, the
# event behind its last launch (None without a GPU), and the id -> string list of a predicting batch (submit(predict=)), else None
Ticket = namedtuple("Ticket", "plan lat topN timing done words")

_READOUT = [False]


def _readout_ext():
    """jlm_amd._readout (built by __graft_entry__.build()), or None; JLM_NATIVE_READOUT=0 disables it."""
    if _READOUT[0] is False:
        ext = None
        if os.environ.get("JLM_NATIVE_READOUT", "1") != "0":
            try:
                from . import _readout as ext
            except ImportError:
                ext = None
        _READOUT[0] = ext
    return _READOUT[0]


def _round_up(x, m):
    return (int(x) + m - 1) // m * m


class _Plan:
    """Device buffers of one decode shape + their torch.classes.jlm.Plan (the C structs of include/jlm_hip.h)."""

    # the four node-sized arrays LAST: lattices built into page-locked blocks (lattice.StagingPool) copy them to the device
    # straight from there, and only the head [0, head_end) goes through this plan's staging block
    BIG_ARRAYS = ("node_start", "node_word", "sg_word", "sg_node")
    INT_ARRAYS = ("sent_len", "end_off", "sg_off", "g0", "cidx", "sidx", "sidx2", "vs_words", "vs_off", "di_words", "di_off", "dd_words",
                  "dd_off")

    def __init__(self, eng, key, caps):
        torch, m, dev = eng.torch, eng.m, eng.device
        self.key, self.caps = key, dict(caps)
        kind, vmode, B, beam, F = key[:5]
        perm = bool(key[6]) if len(key) > 6 else False       # reference-compatibility lists (dynamic x segmented, see submit)
        ctx = bool(key[7]) if len(key) > 7 else False        # a plan for batches with a left context (submit(context=))
        n_pred = int(key[8]) if len(key) > 8 else 0          # a plan for batches whose last word is predicted (submit(predict=)): its n_out
        self.B, self.beam, self.F = B, beam, F
        rmax, ncell = B * beam, F * B
        G = F * rmax
        # the LSTM-step kernels address state rows as 16-byte records through a 31-bit index (csrc/jlm_gate.hip): H / 4 records per row
        # (a plan with a left context keeps the sentences' primed states in B more rows behind the pool: frame 0 reads rows G .. G + B - 1)
        if (G + (B if ctx else 0)) * max(m.H // 4, 1) >= 0x7ffffff0:
            raise ValueError("a decode plan of %d state rows of %d units is beyond the LSTM-step kernels' addressing (rows x H / 4 < 2^31): "
                             "decode fewer sentences per batch (Decoder.max_batch)" % (G, m.H))
        self.rmax, self.G, self.ncell = rmax, G, ncell
        sizes = dict(sent_len=B, end_off=ncell + 1, node_start=caps["nodes"], node_word=caps["nodes"], sg_off=ncell + 1,
                     sg_word=caps["nodes"], sg_node=caps["nodes"], g0=ncell, cidx=ncell, sidx=ncell, sidx2=ncell,
                     vs_words=caps["vs"], vs_off=B + 1, di_words=caps["di"], di_off=2 * ncell, dd_words=caps["dd"],
                     dd_off=ncell + 1)
        names = self.INT_ARRAYS + (("di_wwords", "sg_wword") if perm else ()) + self.BIG_ARRAYS
        if perm:
            sizes.update(di_wwords=caps["di"], sg_wword=caps["nodes"])
        off, self.ioff = 0, {}
        for n in names:
            if n == self.BIG_ARRAYS[0]:
                self.head_end = off
            self.ioff[n] = off
            off += _round_up(max(sizes[n], 1), 4)
        self.isize = {n: sizes[n] for n in names}
        self.host_ints = torch.zeros(off + 4, dtype=torch.int32)
        if dev.type == "cuda":
            self.host_ints = self.host_ints.pin_memory()
        self.host_np = self.host_ints.numpy()
        self.dev_ints = torch.zeros(off + 4, dtype=torch.int32, device=dev)
        # constant index arrays
        self._set("g0", (np.arange(F, dtype=np.int32)[:, None] * rmax + np.arange(B, dtype=np.int32)[None, :] * beam))
        self._set("cidx", np.arange(ncell, dtype=np.int32))
        self._set("sidx", np.tile(np.arange(B, dtype=np.int32), F))
        # the incremental decoder's frame-initial lists are (begin, end) slices of per-sentence sequences
        # (lattice.dynamic_vocab): list number 2 * cell reads its two offsets from di_off[2 * cell .. + 1]
        self._set("sidx2", 2 * np.tile(np.arange(B, dtype=np.int32), F))
        f64, f32, i32 = torch.float64, torch.float32, torch.int32
        dynamic = kind == "dynamic"
        e = lambda n, dt: torch.empty(n, device=dev, dtype=dt)
        self.score, self.lse = e(G, f64), e(G, f64)
        self.ysum = e(G, f64) if dynamic else None
        self.bp, self.node, self.word = e(G, i32), e(G, i32), e(G, i32)
        self.cnt = torch.zeros(ncell, device=dev, dtype=i32)
        self.live = e(G, i32)
        self.live_base = torch.zeros(ncell, device=dev, dtype=i32)
        self.n_live = torch.zeros(F, device=dev, dtype=i32)
        self.edge = e(max(caps["nodes"], 1) * beam, f32)
        H, ldt = m.H, m.ldt
        self.h, self.c = e((G + (B if ctx else 0), H), f32), e((G + (B if ctx else 0), H), f32)
        # untied models: T is the state itself -- the same buffer on the f32 path; with split state rows, their plain f32 copy
        self.T = (e((G, H), f32) if m.split_lstm else self.h) if m.mode == "untied" else e((G, ldt), f32)
        self.run_max = self.run_sum = self.part = None
        self.n_part = 0
        if not m.self_norm:
            if vmode != "full":
                self.run_max, self.run_sum = e(G, f32), e(G, f64)
            else:
                self.n_part = max(m.n_vocab_tiles, 1)
                self.part = e((self.n_part, rmax, 2), f32)
        # packed rows of the frame being stepped, for the segments of the normaliser on mixed rows (jlm_pack_t_mixed)
        self.Tm = None
        if self.part is not None and getattr(m, "ld_tm", 0):
            self.Tm = torch.zeros(((rmax + 31) // 32 * 32, m.ld_tm), device=dev, dtype=f32)      # whole 32-row blocks (granule-major, jlm_hip.h)
        self.stride = F + 1
        self.out_nodes = e((rmax, self.stride), i32)
        self.out_len = torch.zeros(rmax + 1, device=dev, dtype=i32)       # [rmax]: the batch's flag word (jlm_beam_state.flags, ABI 11)
        self.out_score = e(rmax, f64)
        pin = (lambda t: t.pin_memory()) if dev.type == "cuda" else (lambda t: t)
        self.h_nodes = pin(torch.empty((rmax, self.stride), dtype=i32))
        self.h_len = pin(torch.zeros(rmax + 1, dtype=i32))
        self.h_score = pin(torch.empty(rmax, dtype=f64))
        self.h_nlive = pin(torch.empty(F, dtype=i32))
        self.busy = False
        # left context: the root rows' prev / word (seed_context_kernel writes entries s * beam), the batch's rows of the primed state
        self.ctx_prev = self.ctx_word = self.ctx_idx = self.ctx_idx_host = self.ctx_state = None
        self.cache_bufs = None               # decodes under the continuous cache: their score scratch (_CacheBufs), made on first use
        self.ngram_bufs = None               # decodes under an n-gram mixture: the batch's root histories (_NgramBufs), made on first use
        self.memory_bufs = None              # decodes under a memory: one frame's retrieval buffers (_MemoryBufs), made on first use
        self.memory_live = False             # the batch in flight runs under a memory: collect reads the retrieval's flag word
        if ctx:
            self.ctx_prev, self.ctx_word = torch.full((rmax,), -1, device=dev, dtype=i32), torch.zeros(rmax, device=dev, dtype=i32)
            self.ctx_idx, self.ctx_idx_host = torch.zeros(B, device=dev, dtype=i32), pin(torch.zeros(B, dtype=i32))
        # predictions of the last word (jlm_tail_predict): the batch's spans (sp_off [B + 1] | frame | lo | hi, each [caps["spans"]]) and the outputs
        self.n_pred = n_pred
        if n_pred:
            ns, R = caps["spans"], B * n_pred
            self.pr_off = (0, _round_up(B + 1, 4), _round_up(B + 1, 4) + ns, _round_up(B + 1, 4) + 2 * ns, _round_up(B + 1, 4) + 3 * ns)
            self.pr_host = pin(torch.zeros(self.pr_off[-1], dtype=i32))
            self.pr_ints = torch.zeros(self.pr_off[-1], device=dev, dtype=i32)
            self.pr_score, self.pr_row, self.pr_word, self.pr_len = e(R, f64), e(R, i32), e(R, i32), e(R, i32)
            self.pr_nodes = e((R, self.stride), i32)
            self.h_pr_score, self.h_pr_row, self.h_pr_word = pin(torch.empty(R, dtype=f64)), pin(torch.empty(R, dtype=i32)), pin(torch.empty(R, dtype=i32))
            self.h_pr_len, self.h_pr_nodes = pin(torch.empty(R, dtype=i32)), pin(torch.empty((R, self.stride), dtype=i32))
        self.nbytes = sum(t.numel() * t.element_size() for t in vars(self).values() if isinstance(t, torch.Tensor) and t.device == dev)
        # torch.classes.jlm.Plan: the same buffers as jlm_lattice / jlm_beam_state / jlm_decode_plan for the frame-loop op
        tensors = dict(ints=self.dev_ints, score=self.score, lse=self.lse, bp=self.bp, node=self.node, word=self.word,
                       cnt=self.cnt, live=self.live, n_live=self.n_live, live_base=self.live_base, edge=self.edge, h=self.h,
                       c=self.c, T=self.T, out_nodes=self.out_nodes, out_len=self.out_len, out_score=self.out_score)
        for name in ("ysum", "run_max", "run_sum", "part", "Tm", "ctx_prev", "ctx_word"):
            if getattr(self, name) is not None:
                tensors[name] = getattr(self, name)
        ints = dict(n_sent=B, beam=beam, frames=F, kind=2 if dynamic else (1 if vmode == "select" else 0),
                    max_cands=caps["cands"], max_parts=self.n_part, stride=self.stride)
        if self.Tm is not None:
            ints["ld_tm"] = m.ld_tm
        if ctx:
            ints["H"] = H
        ints.update({"off_" + n: o for n, o in self.ioff.items()})
        self.obj = ops.backend().Plan(tensors, ints)

    def _set(self, name, arr):
        arr = np.asarray(arr, dtype=np.int32).reshape(-1)
        assert arr.size <= self.isize[name], (name, arr.size, self.isize[name])
        o = self.ioff[name]
        self.host_np[o:o + arr.size] = arr

    def fits(self, need):
        return all(self.caps[k] >= v for k, v in need.items())


class _CacheBufs:
    """The score scratch of a plan's decodes under the continuous cache: s [rmax, ld_s] float32 (jlm_decode_cache.s), kept on the plan
    and reused while it is wide enough.  Zeroed memory; the kernels write every entry they read."""

    def __init__(self, eng, rmax, ld_s):
        self.ld_s = int(ld_s)
        self.s = eng.torch.zeros((rmax, self.ld_s), device=eng.device, dtype=eng.torch.float32)

    @staticmethod
    def fit(have, eng, rmax, n):
        return have if have is not None and have.ld_s >= n else _CacheBufs(eng, rmax, _round_up(max(n, 1), 64))


class _NgramBufs:
    """What a plan's decodes under an n-gram mixture keep beside the table: root_hist [n_sent, 2] int32 on the device
    (jlm_decode_ngram.root_hist) and its page-locked staging copy, written per batch."""

    def __init__(self, eng, n_sent):
        torch = eng.torch
        self.root_hist = torch.zeros((n_sent, 2), device=eng.device, dtype=torch.int32)
        self.host = torch.zeros((n_sent, 2), dtype=torch.int32)
        if eng.device.type == "cuda":
            self.host = self.host.pin_memory()


class _MemoryBufs:
    """The buffers of one frame's retrieval for a plan's decodes under a memory (jlm_decode_memory): the gathered query rows q_rows
    [rmax, H], the scores s [rmax, K], ret_words [K, rmax], jlm_memory_topk's workspace -- one chunk when the scores of the whole memory
    fit memory.TOPK_SCORE_BYTES (RetrievalBuffers' rule) -- and the retrieval's own flag word with its page-locked copy.  Kept on the plan
    and reused while (N, K) and the chunk stay; all zeroed, none uninitialised."""

    def __init__(self, eng, rmax, N, K):
        torch, dev = eng.torch, eng.device
        self.key = (int(N), int(K), self.CHUNK_KEYS)
        self.q_rows = torch.zeros((rmax, eng.m.H), device=dev, dtype=torch.float32)
        self.s = torch.zeros((rmax, K), device=dev, dtype=torch.float32)
        self.ret_words = torch.full((K, rmax), -1, device=dev, dtype=torch.int32)
        self.workspace = torch.zeros(max(self.workspace_floats(N, rmax, K), 4), device=dev, dtype=torch.float32)
        self.flags = torch.zeros(1, device=dev, dtype=torch.int32)
        self.h_flags = torch.zeros(1, dtype=torch.int32)
        if dev.type == "cuda":
            self.h_flags = self.h_flags.pin_memory()

    CHUNK_KEYS = None        # keys per chunk of the retrieval (None: RetrievalBuffers' rule; tests cut the workspace to chunks of 32)

    @classmethod
    def workspace_floats(cls, N, rmax, K):
        from .memory import RetrievalBuffers
        chunk = RetrievalBuffers.chunk_keys(N, rmax) if cls.CHUNK_KEYS is None else int(cls.CHUNK_KEYS)
        return rmax * (chunk + 2 * K)

    @property
    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in (self.q_rows, self.s, self.ret_words, self.workspace, self.flags))

    @staticmethod
    def fit(have, eng, rmax, N, K):
        return have if have is not None and have.key == (int(N), int(K), _MemoryBufs.CHUNK_KEYS) else _MemoryBufs(eng, rmax, N, K)


class DecodeEngine:
    _stream_pool = {}              # device index -> launch streams shared by all engines of the process
    MAX_PLANS = 6                  # plans kept regardless of their size (up to four are in flight at a time, one is being read out)
    MAX_PLANS_SMALL = 48           # ... and as many more as fit PLAN_BYTES of device memory
    PLAN_BYTES = 4 << 30

    def __init__(self, dev_model):
        self.m = dev_model
        self.torch = dev_model.torch
        self.device = dev_model.device
        self.last_timing = None         # timed decode: (lstm, softmax) seconds per stepped frame (perf_log_* of decoder.py:206-218)
        self.last_fix_timing = None     # ... incremental decoder: (vocab fix, lattice path fix) seconds per frame
        self.last_kernel_ms = None      # ... {"gate_gemm": [...], "vocab_lse": [...]} milliseconds per launch (bench.py)
        self.last_state = None
        self.last_n_live = None
        self.keep_n_live = False        # bench.py: read back every frame's live-row count with a timed decode
        self.use_side = os.environ.get("JLM_SIDE", "1") != "0"       # edge logits beside the normaliser
        self.blocking_sync = False       # (JLM_BLOCKING_SYNC, rounds 2-4: the collecting thread asleep instead of spinning -- no less CPU, 1-3 % slower; removed)
        from .lattice import StagingPool
        self.staging_pool = None if os.environ.get("JLM_PINNED_LATTICE", "1") == "0" else StagingPool(self.torch, self.device.type == "cuda")
        self.plans = []
        # Consecutive batches go to alternating HIP streams: the latency-bound kernels of batch i+1
        # (beam step, LSTM step, T projection: two thirds of the launches, a third of the time, most CUs
        # idle) fill in beside the vocabulary kernel of batch i.  JLM_STREAMS=1 keeps one stream.
        # (round 3: FOUR batches in flight -- 1.95-1.98 against 2.04-2.06 ms per step once the mixed-row normaliser left more of
        # a frame to the latency-bound kernels; five: 2.36 -- Decoder.depth_for keeps three for batches above 8 192 rows)
        # THREE batches in flight on three streams, edge logits on the batch's own stream: 2.14-2.22 ms per step against
        # 2.32-2.36 with two streams + a side stream each (tools/ab_streams.py).  A frame of one batch is a chain of dependent
        # launches (beam step, LSTM step, T projection, vocabulary kernel: every one of them on the critical path of the step,
        # tools/probes/skip_kernel.sh) and the chains of three batches fill each other's gaps better than those of two; side
        # streams on top (six streams, fork / join events across them) cost more than the overlap buys: 3.3 ms.
        # four streams need more than ROCm's default of four hardware queues (one is the null stream's): there they run 2.31 ms per
        # step against 2.06 with three (GPU_MAX_HW_QUEUES >= 8, set by the host process: jlm_amd/__init__.py)
        from . import hw_queues_ok as _hwq
        self.n_streams = max(1, int(os.environ.get("JLM_STREAMS", "4" if _hwq() else "3")))
        # CU share of the vocabulary kernel beside other batches in flight: none since round 4 (the step is flat in it with four batches
        # in flight, profiles/r04_b_share_sweep.txt, and a share below 100 made a score's last bits depend on how many chunks the call
        # had); the JLM_LSE_SHARE knob left in round 5, the frame-loop op keeps its (unused) argument.
        self.lse_share_pct = 100 if self.n_streams >= 2 else 0
        self._streams = []
        self._rr = 0
        # `pipelined`: set by the caller around a pipelined sequence of submits (Decoder.decode_batch).  Per THREAD: two threads inside
        # decode_batch on the same decoder must not clear each other's flag (it decides the CU share, i.e. the vocabulary kernel's
        # column cuts, of every batch the thread submits meanwhile)
        self._tls = threading.local()
        self._submit_lock = threading.RLock()

    @property
    def pipelined(self):
        return getattr(self._tls, "pipelined", False)

    @pipelined.setter
    def pipelined(self, v):
        self._tls.pipelined = bool(v)

    def _ctx(self):
        return self.m._ctx()

    # ------------------------------------------------------------------ plans
    def _plan_for(self, kind, vmode, lat, need, size_class=(), perm=False, ctx=False, n_pred=0):
        # Buffers are sized for the frame count rounded up to 8 so that ragged inputs (every chunk has its own longest
        # sentence) share plans instead of allocating ~1 GB of state rows and pinned staging per distinct length; the
        # frame loop runs lat.n_frames.
        fkey = _round_up(lat.n_frames, 8)
        # (a left context, and a predicted last word, add an element each: every other plan keeps its key)
        key = (kind, vmode, lat.n_sent, lat.beam, fkey, size_class, bool(perm)) + ((bool(ctx),) if (ctx or n_pred) else ()) + \
            ((int(n_pred),) if n_pred else ())
        for i, p in enumerate(self.plans):
            if p.key == key and p.fits(need) and not p.busy:
                self.plans.append(self.plans.pop(i))
                return p
        caps = {k: _round_up(int(v * 1.25) + 64, 1024) for k, v in need.items()}
        # (at least 1 024 where the beam step's LDS takes that many: wide beams over many frames take fewer -- a batch that passed
        #  Decoder._check_cells must also pass the launcher's LDS formula)
        lim = int(ops.backend().beam_step_max_cands(int(lat.beam), fkey, 2 if kind == "dynamic" else (1 if self.m.self_norm else 0)))
        caps["cands"] = max(_round_up(need["cands"], 256), min(1024, lim) if lim > 0 else 1024)
        self.plans = [p for p in self.plans if p.busy or p.key != key or p.fits(need)]
        p = _Plan(self, key, caps)
        # Least recently used idle plans go when the set outgrows its budget: a count for the big batch plans (hundreds
        # of MB each), bytes for the small ones -- sentence-at-a-time callers (eval.py) meet a new (length bucket, list
        # size) shape every few calls, and re-allocating a plan costs more than the decode it serves.
        idle = [q for q in self.plans if not q.busy]
        total = sum(q.nbytes for q in self.plans) + p.nbytes
        while idle and (len(self.plans) >= self.MAX_PLANS_SMALL or
                        (total > self.PLAN_BYTES and len(self.plans) >= self.MAX_PLANS)):
            q = idle.pop(0)
            self.plans.remove(q)
            total -= q.nbytes
        self.plans.append(p)
        return p

    # ----------------------------------------------------------------- decode
    def ngram_tensors(self, table):
        """the device tensors of an NGramTable's hash table -- (keys int64 [2^log2cap], vals float32 [2^log2cap, 2], its
        device_arrays()) --, made once per table and device and reused by every batch"""
        key = (self.device.type, self.device.index)
        if key not in table._dev:
            arr = table.device_arrays()
            torch = self.torch
            with self._ctx():
                table._dev[key] = (torch.from_numpy(arr["keys"].view(np.int64)).to(self.device), torch.from_numpy(arr["vals"]).to(self.device), arr)
        return table._dev[key]

    def submit(self, lat, kind="static", vocab=None, dyn_lists=None, topN=10, timing=False, context=None, predict=None, ngram=None,
               memory=None):
        """Enqueue one batch (upload, the frame-loop op, asynchronous read-back) and return a
        ticket for :meth:`collect`.  Nothing here waits for the GPU.  Successive calls use
        alternating streams (see __init__); every ticket owns its plan's buffers until collected.
        timing=True: HIP events around the kernel groups of every frame (one stream, no side stream);
        timing="inflight": the same events recorded on the batch's own stream of the PIPELINED submit -- a kernel's time
        then includes what it loses to the other batches in flight (bench.py: `frac_in_pipeline`).
        context: None, or (ContextState, the state's row of every sentence of ``lat``): the sentences' primed states are gathered behind
        the plan's pool by one launch in front of the frame loop, on the batch's stream (jlm_amd/context.py).  A CachedContext with
        lam > 0 also hands the frame loop every sentence's window (``torch.ops.jlm.seed_cache``: no launch): the continuous cache is
        mixed into every edge cost (static full-vocabulary decodes only, ValueError otherwise).
        predict: None, or ((sp_off [n_sent + 1], sp_frame, sp_lo, sp_hi), ids, words, n_out): the batch's spans in CSR (sentence s: the
        frames its unfinished tail may start at and the range of ``ids`` -- the device copy of ReadingIndex.ids -- of the words whose
        reading properly extends the tail from there), ``words`` the id -> string list; one more launch behind the frame loop
        (jlm_tail_predict) selects the n_out best (hypothesis, extension word) pairs per sentence, and :meth:`collect` returns
        (conversions, predictions) pairs (static full-vocabulary decodes only).
        ngram: None, or a jlm_amd.ngram.NGramMix: the back-off n-gram model is mixed into every edge cost (``torch.ops.jlm.seed_ngram``:
        no launch; one more launch per frame, csrc/jlm_ngram_edge.hip).  Static full-vocabulary decodes only and
        not under the continuous cache: ValueError otherwise.
        memory: None, or a jlm_amd.memory.MemoryMix of this model with lam > 0: the mass of every row's K nearest entries is mixed into
        every edge cost (``torch.ops.jlm.seed_memory``: no launch; per frame a gather, jlm_memory_topk and a patch,
        csrc/jlm_memory_edge.hip), with or without ``context``.  Static full-vocabulary decodes of at most 65 535
        rows only, and not beside the continuous cache or an n-gram mixture: ValueError otherwise."""
        torch = self.torch
        with self._submit_lock, self._ctx():          # (the plan list and the stream rotation are shared by every submitting thread)
            if self.device.type != "cuda" or self.n_streams < 2 or (timing and timing != "inflight"):
                return self._submit(lat, kind, vocab, dyn_lists, topN, timing, context, predict, ngram, memory)
            if len(self._streams) != self.n_streams:
                # the launch streams are shared by every engine on the device: each also gets a side stream inside the op, and
                # streams beyond the GPU's hardware queues (GPU_MAX_HW_QUEUES, jlm_amd/__init__.py) serialise one another --
                # a second Decoder in the process (bench.py's configs[4] leg) must not double them
                pool = DecodeEngine._stream_pool.setdefault(self.device.index or 0, [])
                while len(pool) < self.n_streams:
                    pool.append(torch.cuda.Stream(self.device))
                self._streams = pool[:self.n_streams]
            strm = self._streams[self._rr]
            self._rr = (self._rr + 1) % self.n_streams
            cur = torch.cuda.current_stream(self.device)
            if not cur.query():                                  # after whatever the caller queued (weight uploads, ...);
                strm.wait_stream(cur)                            # nothing pending there in the steady state: no event, no wait
            with torch.cuda.stream(strm):
                return self._submit(lat, kind, vocab, dyn_lists, topN, timing, context, predict, ngram, memory)

    def _submit(self, lat, kind, vocab, dyn_lists, topN, timing, context=None, predict=None, ngram=None, memory=None):
        torch = self.torch
        dynamic = kind == "dynamic"
        vmode = "dynamic" if dynamic else ("select" if vocab is not None else "full")
        need = dict(nodes=lat.n_nodes, vs=len(vocab[0]) if vocab is not None else 0,
                    di=len(dyn_lists[0]) if dynamic else 0, dd=len(dyn_lists[2]) if dynamic else 0, cands=lat.max_cands)

        # longest word list per kind of call (selected vocabulary / frame-initial / frame-delta lists): which
        # kernel a call uses depends on it
        def longest(offs):
            o = np.asarray(offs)
            return int(np.diff(o).max()) if o.size > 1 else 0
        max_words = dict(vs=longest(vocab[1]) if vocab is not None else 0,
                         di=int((dyn_lists[1][1::2] - dyn_lists[1][0::2]).max()) if dynamic else 0,
                         dd=longest(dyn_lists[3]) if dynamic else 0)
        size_class = tuple((v < 128, v <= 128, v <= 4064) for v in (max_words["vs"], max_words["di"], max_words["dd"]))
        # dyn_lists[4:6] (optional): the weight-row words of the reference-compatibility mode (DynamicDecoder.compat_quirks on
        # D-softmax / D-softmax* models): per init-list position and per lattice edge (include/jlm_hip.h, jlm_decode_plan)
        perm = dynamic and len(dyn_lists) >= 6 and dyn_lists[4] is not None
        if context is not None:
            state, rows = context
            rows = np.asarray(rows, dtype=np.int32).reshape(-1)
            if state.m is not self.m or rows.shape[0] != lat.n_sent or (rows.size and (rows.min() < 0 or rows.max() >= state.n)):
                raise ValueError("context: one row of a ContextState of this model per sentence of the batch")
        cached = context is not None and getattr(state, "spec", None) is not None and state.spec.lam > 0.0
        if cached and (dynamic or vocab is not None or predict is not None):
            raise ValueError("the continuous cache runs inside the static full-vocabulary decode only")
        if ngram is not None:
            from .ngram import check_mix
            check_mix(ngram, self.m.V)
            if dynamic or vocab is not None or predict is not None:
                raise ValueError("an n-gram mixture runs inside the static full-vocabulary decode only")
            if cached:
                raise ValueError("an n-gram mixture and the continuous cache in one decode: a three-way mixture is not defined")
        if memory is not None:
            from .memory import _check_mix
            _check_mix(self.m, memory)
            if not memory.lam > 0.0:
                raise ValueError("memory: lam = 0 is the decode without a memory (pass memory=None)")
            if dynamic or vocab is not None or predict is not None:
                raise ValueError("a memory runs inside the static full-vocabulary decode only")
            if cached or ngram is not None:
                raise ValueError("a memory beside the continuous cache or an n-gram mixture: a three-way mixture is not defined")
            if lat.n_sent * lat.beam > 65535:
                raise ValueError("a decode under a memory takes at most 65535 rows a batch (n_sent x beam = %d x %d)" % (lat.n_sent, lat.beam))
        if predict is not None:
            if dynamic or vocab is not None:
                raise ValueError("predict: the last word is predicted behind a static full-vocabulary decode only")
            sp = [np.asarray(a, dtype=np.int32).reshape(-1) for a in predict[0]]
            n_pred = int(predict[3])
            if not 1 <= n_pred <= 64 or sp[0].shape[0] != lat.n_sent + 1 or not (sp[1].shape == sp[2].shape == sp[3].shape) or \
                    int(sp[0][0]) != 0 or int(sp[0][-1]) != sp[1].shape[0] or (np.diff(sp[0]) < 0).any():
                raise ValueError("predict: n_out is 1 .. 64, the spans are CSR over the batch's sentences")
            sent_of = np.repeat(np.arange(lat.n_sent), np.diff(sp[0]))
            if sp[1].size and (sp[1].min() < 0 or (sp[1] >= np.asarray(lat.sent_len)[sent_of]).any() or (sp[2] > sp[3]).any()):
                raise ValueError("predict: a span's frame lies inside its sentence (0 <= frame < length), its words are ids[lo:hi]")
            # a sentence's candidate index is an int32 on the device
            per = np.zeros(lat.n_sent, dtype=np.int64)
            np.add.at(per, sent_of, (sp[3] - sp[2]).astype(np.int64))
            if int(per.max()) * lat.beam >= 2 ** 31:
                raise ValueError("predict: a sentence has 2^31 or more (hypothesis, word) candidates")
            need["spans"] = int(sp[1].shape[0])
        p = self._plan_for(kind, vmode, lat, need, size_class, perm, ctx=context is not None, n_pred=n_pred if predict is not None else 0)
        p.busy = True
        p.memory_live = memory is not None
        try:
            if context is not None:
                # the primed rows of this batch's sentences -> rows G + s of the plan's pool, prev / word of the root rows: one launch
                p.ctx_state = state          # (kept until the batch is collected: the gather reads it on this stream)
                p.ctx_idx_host.numpy()[:] = rows
                p.ctx_idx.copy_(p.ctx_idx_host, non_blocking=True)
                ops.backend().seed_context(p.obj, state.h, state.c, state.last, state.has, p.ctx_idx)
                if cached:
                    # the window of every sentence for this frame loop (jlm_decode_plan.cache): no launch, the op keeps the tensors
                    p.cache_bufs = bufs = _CacheBufs.fit(p.cache_bufs, self, p.rmax, min(state.cap, state.spec.size))
                    ops.backend().seed_cache(p.obj, state.hist, state.words, state.count, p.ctx_idx, bufs.s, int(state.cap),
                                             int(state.spec.size), float(state.spec.theta), float(state.spec.lam))
            if ngram is not None:
                # the table and every sentence's root history for this frame loop (jlm_decode_plan.ngram): one small upload, no launch
                from .generate import EOS_ID
                if p.ngram_bufs is None:
                    p.ngram_bufs = _NgramBufs(self, p.B)
                nb, root = p.ngram_bufs, p.ngram_bufs.host.numpy()
                root[:] = 0
                root[:lat.n_sent] = (-1, EOS_ID) if context is None else state.tail_host[rows]
                nb.root_hist.copy_(nb.host, non_blocking=True)
                keys, vals, arr = self.ngram_tensors(ngram.table)
                ops.backend().seed_ngram(p.obj, keys, vals, nb.root_hist, int(arr["log2cap"]), int(arr["max_probe"]), int(ngram.table.order),
                                         float(ngram.lam))
            if memory is not None:
                # the memory and one frame's retrieval buffers for this frame loop (jlm_decode_plan.memory): no launch, no upload
                mem = memory.memory
                p.memory_bufs = mb = _MemoryBufs.fit(p.memory_bufs, self, p.rmax, mem.N, memory.k)
                mb.flags.zero_()
                ops.backend().seed_memory(p.obj, mem.keys, mem.words, int(mem.N), int(self.m.H), float(memory.theta), float(memory.lam),
                                          int(memory.k), mb.q_rows, mb.s, mb.ret_words, mb.workspace, mb.flags)
            done = self._enqueue(p, lat, vocab, dyn_lists, dynamic, perm, max_words, topN, timing)
            if memory is not None:
                mb.h_flags.copy_(mb.flags, non_blocking=True)
                if self.device.type == "cuda":
                    done = torch.cuda.Event(blocking=self.blocking_sync)
                    done.record()
            if predict is not None:
                done = self._enqueue_predict(p, sp, predict[1], n_pred)
        except BaseException:
            if cached:
                ops.backend().clear_cache(p.obj)      # (the window was for this batch's frame loop, which may not have run)
            if ngram is not None:
                ops.backend().clear_ngram(p.obj)
            if memory is not None:
                ops.backend().clear_memory(p.obj)
            # nothing may keep the plan: launches already enqueued finish first, then its buffers are free again
            if self.device.type == "cuda":
                try:
                    torch.cuda.current_stream(self.device).synchronize()
                except Exception:
                    pass
            p.busy = False
            raise
        return Ticket(p, lat, topN, timing, done, predict[2] if predict is not None else None)

    PREDICT_CHUNK = 0        # jlm_tail_predict's `chunk` (0: the launcher's default; tests move the chunk boundary)

    def _enqueue_predict(self, p, sp, ids, n_pred):
        """the spans' upload, jlm_tail_predict and the read-back of its outputs, behind the batch's frame loop on the same stream"""
        torch = self.torch
        o, h = p.pr_off, p.pr_host.numpy()
        h[:sp[0].shape[0]] = sp[0]
        for k in (1, 2, 3):
            h[o[k]:o[k] + sp[k].shape[0]] = sp[k]
        p.pr_ints.copy_(p.pr_host, non_blocking=True)
        ops.backend().tail_predict(self.m.decode_model(), p.obj, ids, p.pr_ints[o[0]:o[1]], p.pr_ints[o[1]:o[2]], p.pr_ints[o[2]:o[3]],
                                   p.pr_ints[o[3]:o[4]], int(n_pred), int(self.PREDICT_CHUNK), p.pr_score, p.pr_row, p.pr_word, p.pr_nodes,
                                   p.pr_len, int(p.stride))
        for dst, src in ((p.h_pr_score, p.pr_score), (p.h_pr_row, p.pr_row), (p.h_pr_word, p.pr_word), (p.h_pr_len, p.pr_len),
                         (p.h_pr_nodes, p.pr_nodes)):
            dst.copy_(src, non_blocking=True)
        done = None
        if self.device.type == "cuda":
            done = torch.cuda.Event(blocking=self.blocking_sync)
            done.record()
        return done

    def _enqueue(self, p, lat, vocab, dyn_lists, dynamic, perm, max_words, topN, timing):
        torch = self.torch
        assert lat.n_frames <= p.F
        p._set("sent_len", lat.sent_len)
        p._set("end_off", lat.end_off)
        p._set("sg_off", lat.sg_off)
        blk = getattr(lat, "_block", None)
        if blk is None:
            for name in p.BIG_ARRAYS:
                p._set(name, getattr(lat, name))
        if vocab is not None:
            p._set("vs_words", vocab[0])
            p._set("vs_off", vocab[1])
        if dynamic:
            p._set("di_words", dyn_lists[0])
            p._set("di_off", dyn_lists[1])
            p._set("dd_words", dyn_lists[2])
            p._set("dd_off", dyn_lists[3])
            if perm:
                p._set("di_wwords", dyn_lists[4])
                p._set("sg_wword", dyn_lists[5])
        be = ops.backend()
        from . import hw_queues_ok
        side = self.use_side and self.device.type == "cuda" and (
            self.n_streams < 2 or (self.n_streams == 2 and hw_queues_ok()) or os.environ.get("JLM_SIDE") == "1")
        share = self.lse_share_pct if ((not timing or timing == "inflight") and self.pipelined and self.lse_share_pct < 100) else 0
        if self.device.type == "cuda" and hasattr(be, "decode_batch"):
            # Round 5: upload, counters, frame loop and read-back of the batch as ONE op (csrc/jlm_torch_ops.cpp decode_batch) -- the
            # dozen torch calls below cost the calling thread 0.3-0.6 ms of interpreter time per 256-sentence chunk
            # (profiles/r05_i_host_profile.txt), the op runs without the interpreter lock
            src, dst, cnt = [], [], []
            if blk is not None:
                for name in p.BIG_ARRAYS:
                    n = int(getattr(lat, name).shape[0])
                    assert n <= p.isize[name], (name, n, p.isize[name])
                    src.append(int(lat.block_off[name])); dst.append(int(p.ioff[name])); cnt.append(n)
            rc = be.decode_batch(self.m.decode_model(), p.obj, p.host_ints, int(p.head_end) if blk is not None else 0,
                                 blk.tensor if blk is not None else None, src, dst, cnt, p.h_nodes, p.h_len, p.h_score,
                                 p.h_nlive if (timing and self.keep_n_live) else None, lat.n_frames, max_words["vs"], max_words["di"],
                                 max_words["dd"], bool(side), bool(timing), int(share))
            if rc != 0:
                raise _lib.JlmHipError("jlm.decode_batch: the model is outside the shapes the frame loop covers (code %d)" % rc)
            done = torch.cuda.Event(blocking=self.blocking_sync)
            done.record()
            return done
        if blk is None:
            p.dev_ints.copy_(p.host_ints, non_blocking=True)
        else:
            # the head from the plan's staging block, the node arrays straight from the lattice's page-locked block
            p.dev_ints[:p.head_end].copy_(p.host_ints[:p.head_end], non_blocking=True)
            for name in p.BIG_ARRAYS:
                n, o, d = int(getattr(lat, name).shape[0]), lat.block_off[name], p.ioff[name]
                assert n <= p.isize[name], (name, n, p.isize[name])
                if n:
                    p.dev_ints[d:d + n].copy_(blk.tensor[o:o + n], non_blocking=True)
        p.cnt.zero_()
        p.n_live.zero_()
        p.out_len[-1:].zero_()          # the flag word
        # (side stream for the edge logits -- `side` above: with one stream, and with two when the hardware queues are there (ROCm's default
        #  of four is not enough: jlm_amd/__init__.py); with three or more streams (the default is four) they run on the batch's own stream)
        # the whole launch sequence of the batch: ONE op, no host synchronisation inside (csrc/jlm_decode.hip)
        # another batch in flight: this batch's vocabulary kernel takes LSE_SHARE_PCT of the CUs and the other batch's
        # latency-bound kernels the rest, side by side (include/jlm_hip.h, jlm_decode_plan.lse_cu_share_pct)
        # The share is a property of the CALL (a pipelined sequence of batches: decode_batch with more than one chunk sets
        # `pipelined`), not of what happens to be in flight at this moment: the share moves the column cuts of the vocabulary
        # kernel, i.e. the grouping of its f32 partial sums, and a sentence's score must not depend on its chunk's position.
        rc = be.decode_frames(self.m.decode_model(), p.obj, lat.n_frames, max_words["vs"], max_words["di"],
                                         max_words["dd"], bool(side), bool(timing), int(share))
        if rc != 0:
            raise _lib.JlmHipError("jlm.decode_frames: the model is outside the shapes the frame loop covers (code %d)" % rc)
        p.h_nodes.copy_(p.out_nodes, non_blocking=True)
        p.h_len.copy_(p.out_len, non_blocking=True)
        p.h_score.copy_(p.out_score, non_blocking=True)
        if timing and self.keep_n_live:
            p.h_nlive.copy_(p.n_live, non_blocking=True)
        done = None
        if self.device.type == "cuda":
            # JLM_BLOCKING_SYNC=1: the collecting thread sleeps until the batch is done instead of spinning on the event
            # (measured: no less CPU per step -- the runtime's own threads spin either way -- and 1-3 % more wall time: off)
            done = torch.cuda.Event(blocking=self.blocking_sync)
            done.record()
        return done


    def collect(self, ticket, keep=False):
        """Wait for a submitted batch and build its n-best lists.  keep=True: the plan stays busy -- its pools are read once more
        (:meth:`candidates`) -- and the caller clears ``ticket.plan.busy``; a batch that fails here leaves no plan busy either way."""
        p, lat, timing, done = ticket.plan, ticket.lat, ticket.timing, ticket.done
        with self._ctx():
            if done is not None:
                done.synchronize()
            if timing:
                t = ops.backend().frame_times(p.obj).numpy() * 1e-3          # [frames, 5] seconds
                stepped = t[:-1]                                                 # the last frame is not stepped
                self.last_timing = [(float(r[2]), float(r[3] + r[4])) for r in stepped]
                self.last_fix_timing = [(float(r[0]), float(r[1])) for r in t]
                self.last_kernel_ms = {"gate_gemm": (stepped[:, 2] * 1e3).tolist(), "vocab_lse": (stepped[:, 4] * 1e3).tolist()}
                if self.keep_n_live:
                    self.last_n_live = p.h_nlive.numpy()[:lat.n_frames].copy()
        self.last_state = p
        p.ctx_state = None
        if p.memory_live and int(p.memory_bufs.h_flags[0]) != 0:
            p.busy = False
            from .memory import _flag_error
            raise _flag_error(int(p.memory_bufs.h_flags[0]))
        if int(p.h_len[-1]) != 0:
            # (ABI 11) the beam step met a log-normaliser that is not finite: a row's sum of 2^y overflowed (or vanished) in the fixed-reference
            # normaliser -- an overflowed row's hypotheses would score -inf and be pruned, leaving a plausible but wrong n-best
            p.busy = False
            if int(p.h_len[-1]) & 8:
                raise _lib.JlmHipError("the cache flagged a product h . h_i that is not finite: a hidden state is NaN or inf (or, under an "
                                       "n-gram mixture, a hypothesis's score is not finite)")
            raise _lib.JlmHipError("a log-normaliser is not finite: this model's logits left the range the fixed-reference normaliser covers "
                                   "(DeviceModel.mixed_calib); set JLM_MX_FIXREF=0")
        if getattr(self.m, "lse_fixed_ref", 0):
            # the normaliser ran without a running maximum (jlm_vocab_lse_mixed_fr): a row whose logits left the range the load-time probe
            # vouched for comes back as log 0 or log inf -- never a plausible score.  Loud, not silent:
            sc, ln = p.h_score.numpy(), p.h_len.numpy()[:-1]
            if not np.isfinite(sc[ln > 0]).all():
                p.busy = False
                raise _lib.JlmHipError("a path score is not finite: this model's logits left the range the fixed-reference normaliser covers "
                                       "(DeviceModel.mixed_calib); set JLM_MX_FIXREF=0")
        out = self._read_out(lat, p.h_nodes.numpy(), p.h_len.numpy()[:-1], p.h_score.numpy(), ticket.topN)
        if ticket.words is not None:
            out = list(zip(out, self._read_predictions(lat, p, ticket.words)))
        if not keep:
            p.busy = False
        return out

    ALT_MAX_ROWS = None      # rows per jlm_alt_frames call (None: score.MAX_ROWS within score.SCORE_BUDGET_BYTES; tests force it down)

    def candidates(self, ticket, rank=0, lookahead=None, n_cand=10):
        """The per-segment candidate lists of path ``rank`` of a collected static full-vocabulary batch whose plan is still busy
        (collect(keep=True)): -> per sentence [(start, length, [(score, word), ...])] (jlm_amd/candidates.py).
        Per call of at most ALT_MAX_ROWS rows ONE op (``torch.ops.jlm.alt_frames``): the head launch over the plan's pools, then
        score_frames' launches for the longest suffix, no host synchronisation inside, on the caller's current stream: collect() has waited
        for the decode, so it need not be the decode's stream.  The row sets and id arrays are the call's own."""
        from . import candidates as _cand
        from . import score as _score
        from .rowsets import RowSets, check_ids, clamp_rows
        p, lat, m, torch = ticket.plan, ticket.lat, self.m, self.torch
        if not p.busy or p.key[0] != "static" or p.key[1] != "full":
            raise ValueError("candidates: a collected static full-vocabulary batch whose plan is still held (collect(keep=True))")
        segments = _cand.segments_of(lat, p.h_nodes.numpy(), p.h_len.numpy()[:-1], int(rank))
        longest = max((len(sg) for sg in segments), default=0)
        max_rows = self.ALT_MAX_ROWS or clamp_rows(_score.MAX_ROWS, _score.SCORE_BUDGET_BYTES,
                                                   _score.Scorer(m).row_bytes(max(longest - 1, 0), per_token=False), m.H)
        index, calls = _cand.plan_rows(lat, segments, lookahead, int(max_rows))
        totals = np.zeros(len(index), dtype=np.float64)
        dev, f64, i32 = self.device, torch.float64, torch.int32
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        with self._ctx():
            for call in calls:
                R, S = len(call["idx"]), int(call["n_steps"])
                check_ids(call["alt"], m.V, "candidates")
                check_ids(call["target"], m.V, "candidates")
                rs = RowSets(m, R)
                part, n_parts, Tm = None, 0, None
                if not m.self_norm:
                    n_parts = max(m.n_vocab_tiles, 1)
                    part = torch.zeros((n_parts, R, 2), device=dev, dtype=torch.float32)
                    if getattr(m, "ld_tm", 0):
                        Tm = torch.zeros(((R + 31) // 32 * 32, m.ld_tm), device=dev, dtype=torch.float32)     # whole 32-row blocks (jlm_hip.h)
                # The head launch writes prev0 and the accumulator of every row a sentence lists -- all of them -- and the normaliser every
                # slice it reads: none of the three needs a value.  They are filled all the same: every uninitialised allocation of the
                # package is a site the poison modules must reach, and a row the head launch skipped then reads as
                # prev0 = -1 / total 0.0, which tests/test_gpu_alt_head.py pins on poisoned buffers.  (part: n_vocab_tiles x rows x 8 bytes a call.)
                prev0 = torch.full((R,), -1, device=dev, dtype=i32)
                nll_seq = torch.zeros(R, device=dev, dtype=f64)
                n_live = [int(x) for x in call["n_live"]]
                ops.backend().alt_frames(m.decode_model(), p.obj, int(rank), up(call["sent_off"]), up(call["sent_rows"]), up(call["depth"]),
                                         up(call["alt"]), *rs.state(), Tm, int(m.ld_tm or 0), part, n_parts, rs.rows, prev0,
                                         up(call["word"]), up(call["target"]), up(call["n_live"]), n_live, nll_seq, None, rs.flags, R, S,
                                         False)
                fl = int(rs.flags.cpu()[0])
                if fl & 4:
                    raise _lib.JlmHipError("candidates: a path's back-pointer chain left the plan's pools (flags %d)" % fl)
                rs.check_flags("candidates: a word outside the model's segments (flags %d)",
                               "a log-normaliser is not finite: this model's logits left the range the fixed-reference normaliser covers "
                               "(DeviceModel.mixed_calib); set JLM_MX_FIXREF=0")
                totals[call["idx"]] = nll_seq.cpu().numpy()
        return _cand.lists_of(lat, segments, index, totals, int(n_cand))

    @staticmethod
    def _read_predictions(lat, p, words):
        """[(score, [word, ...])] per sentence from jlm_tail_predict's outputs: the parent's trace (root dropped, as the n-best read-out drops
        it) followed by the extension word; a sentence's list ends at its first padded rank"""
        n = p.n_pred
        score, row, word = p.h_pr_score.numpy(), p.h_pr_row.numpy(), p.h_pr_word.numpy()
        ln, nodes = p.h_pr_len.numpy(), p.h_pr_nodes.numpy()
        out = []
        for s in range(lat.n_sent):
            lst = []
            for o in range(s * n, (s + 1) * n):
                if row[o] < 0:
                    break
                path = lat.words_of(nodes[o, :max(int(ln[o]) - 1, 0)][::-1]).tolist() if ln[o] > 1 else []
                lst.append((float(score[o]), path + [words[int(word[o])]]))
            out.append(lst)
        return out

    def decode(self, lat, kind="static", vocab=None, dyn_lists=None, topN=10, timing=False, keep_state=False):
        """lat: BatchLattice.  kind: 'static' | 'dynamic'.
        vocab: (words, off) CSR of per-sentence selected vocabularies (static
        vocab_select) or None for the full vocabulary.
        dyn_lists: (seq_words, init_range, delta_words, delta_off) for 'dynamic' (BatchLattice.dynamic_vocab).
        -> list (per sentence) of [(neg_log_prob, [word, ...])][:topN]"""
        if lat.n_sent == 0:
            return []
        return self.collect(self.submit(lat, kind, vocab, dyn_lists, topN, timing))

    @staticmethod
    def _read_out(lat, nodes_h, len_h, score_h, topN):
        """n-best lists of the batch from the back-traces: [(score, [word, ...])] per sentence, best first.
        Built by the C extension jlm_amd._readout (csrc/jlm_readout.c: 0.4 ms for 2 560 paths) when it is
        there, else by the numpy implementation below (1.8 ms) -- same result, tests/test_readout.py."""
        ext = _readout_ext()
        if ext is None:
            return DecodeEngine._read_out_py(lat, nodes_h, len_h, score_h, topN)
        i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
        nodes_h = i32(nodes_h)
        return ext.nbest(nodes_h, i32(len_h), np.ascontiguousarray(score_h, dtype=np.float64), i32(lat.node_lex),
                         i32(lat.node_sent), i32(lat.node_start), lat.builder.lex_list, lat.texts, lat.n_sent, lat.beam,
                         int(topN), nodes_h.shape[-1])

    @staticmethod
    def _read_out_py(lat, nodes_h, len_h, score_h, topN):
        """numpy form of _read_out: one gather of all paths' node ids, one node -> string lookup, two tolist() calls."""
        B, beam = lat.n_sent, lat.beam
        R = min(beam, topN)
        ln = np.asarray(len_h).reshape(B, beam)[:, :R]
        # ranks are filled from 0; a sentence's list ends at its first empty rank
        valid = np.logical_and.accumulate(ln > 0, axis=1)
        nrank = valid.sum(axis=1)
        rows = (np.arange(B)[:, None] * beam + np.arange(R)[None, :])[valid]          # path rows, sentence-major
        k = ln[valid].astype(np.int64) - 1                                             # words per path (root dropped)
        kmax = int(k.max()) if k.size else 0
        flat_words = []
        if kmax > 0:
            cols = np.arange(kmax)[None, :]
            keep = cols < k[:, None]
            src = np.where(keep, k[:, None] - 1 - cols, 0)                             # reversed: last word first in the trace
            ids = np.take_along_axis(np.asarray(nodes_h)[rows][:, :max(kmax, 1)], src, axis=1)[keep]
            flat_words = lat.words_of(ids).tolist()
        ends = np.cumsum(k).tolist()
        scores = np.asarray(score_h)[rows].tolist()
        out, p, a = [], 0, 0
        for s in range(B):
            lst = []
            for _ in range(int(nrank[s])):
                e = ends[p]
                lst.append((scores[p], flat_words[a:e]))
                a = e
                p += 1
            out.append(lst)
        return out
