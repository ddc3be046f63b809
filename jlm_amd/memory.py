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
from .cache import CacheSpec, decode_rows, mix_nll
from .rowsets import check_streams, is_int
from .score import MAX_ROWS, SCORE_BUDGET_BYTES, sentence_loop

MAX_KEYS = 1 << 24                  # JLM_MEMORY_MAX_KEYS
MIN_SPLIT_KEYS = 512                # JLM_MEMORY_MIN_SPLIT_KEYS
MAX_SPLITS = 128                    # JLM_MEMORY_MAX_SPLITS


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
