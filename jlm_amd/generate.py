"""Batched ancestral sampling on the device: ``LSTM_Model.generate`` and ``python -m jlm_amd.generate``.

The reference checks a language model by sampling from it: decoder/model.py:213-245 starts at ``<eos>`` and draws words one
``predict()`` at a time with ``sample(pred, temperature)`` (model.py:28-33), and train/test.py is an interactive form of the same
check.  Here one call is ONE op (``torch.ops.jlm.generate_frames``, csrc/jlm_decode.hip ``jlm_generate_frames``) over many rows: per
frame the LSTM step, the T projection, the full-vocabulary logits (``jlm_gemm_nt`` per segment) and ``sample_rows_kernel``
(csrc/jlm_score.hip), which draws each row's next word by an inverse CDF in word-id order and feeds it to the next frame on the device.

Semantics (pinned by tests/test_generate_cpu.py and tests/test_gpu_generate.py):
  - row r starts from the zero state, consumes its prompt teacher-forced, then draws ``n_words`` words, each from
    softmax(y / temperature) over the full vocabulary (temperature 0: the argmax, the lowest id winning a tie);
  - draw ``step`` of row ``row`` (its index in the caller's list) uses u = :func:`uniform` (seed, step, row), so the result does not
    depend on how rows are cut into calls or on the other rows' prompts;
  - nll is the draw's -log p at temperature 1 (score()'s convention: lse - y, -y for self-normalised models).

Truncation (``top_k``, ``top_p``; pinned by tests/test_generate_truncated_cpu.py and tests/test_gpu_generate_truncated.py).  With
the masses w_j = expf((y_j - max y) * (float)(1 / temperature)) of the plain draw, and words ranked by (y_j descending, word id
ascending) -- a rank order of the logits, so it does not depend on the temperature:
  - ``top_k = k`` (integer >= 1): the kept set K is the first min(k, V) words in rank order; None or k >= V: off;
  - ``top_p = p`` (0 < p <= 1): within K, the shortest prefix in rank order whose mass is >= p * mass(K), at least one word; None or
    p >= 1: off.  Top-k is applied first, then top-p on what it kept;
  - the draw is the same inverse CDF in word-id order over the kept words only, with the same u: the smallest kept i with
    sum_{kept j <= i} w_j > u * S_kept (the last kept word with mass when rounding leaves no crossing);
  - temperature 0 is greedy whatever k and p are; ``top_k = 1`` is the same argmax, the lowest id winning a tie;
  - nll is unchanged: the draw's -log p under the FULL distribution at temperature 1, so it stays comparable with score();
  - as before, a draw depends on (seed, step, the caller's row index) only, and is bit-identical run to run.
The draws are then ``torch.ops.jlm.generate_frames_trunc`` (``jlm_generate_frames_trunc``, ``sample_rows_trunc_kernel``); with both
off the call is the plain ``generate_frames`` op with the arguments it always had.

Prompts are right-aligned: rows are sorted by prompt length, longest first, so the rows a prompt frame steps are a prefix and every
row draws at the same frames.
"""
import argparse
import sys
import time

import numpy as np

from . import config as _config
from . import ops as _ops
from . import rowsets
from .rowsets import check_ids, prompt_arrays
from .rowsets import plan_prompts as plan_rows     # one row per prompt

# the logit buffer is rows x V x 4 bytes (V = 100 k: 1 GB at 2 560 rows); 2 560 rows fill the logit GEMM's tiles on every CU
MAX_ROWS = 2560
GENERATE_BUDGET_BYTES = 3 << 29
# <eos>: index 1 of both Vocab and CharVocab (the lexicon's first entry, behind <unk>; jlm_amd/data.py) -- the reference's starting_text
EOS_ID = 1

_M64 = (1 << 64) - 1


def uniform(seed, step, row):
    """The draw's uniform u in (0, 1): splitmix64 of a (step, row) counter (include/jlm_hip.h jlm_sample_rows).  numpy-broadcasting
    over ``step`` and ``row``; -> float64 array."""
    with np.errstate(over="ignore"):
        step = np.asarray(step, dtype=np.uint64)
        row = np.asarray(row, dtype=np.uint64)
        z = np.uint64(int(seed) & _M64) + np.uint64(0x9E3779B97F4A7C15) * ((step << np.uint64(32)) | (row + np.uint64(1)))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return ((z >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53


def inverse_cdf(mass, u):
    """The draw for masses ``mass`` (one row, word-id order) and u: the smallest i with cumsum(mass)[i] > u * sum(mass); the last word
    with non-zero mass when rounding leaves no crossing."""
    c = np.cumsum(np.asarray(mass, dtype=np.float64))
    i = int(np.searchsorted(c, u * c[-1], side="right"))
    if i >= len(c):
        i = int(np.nonzero(np.asarray(mass) > 0)[0][-1])
    return i


def kept_mask(y, temperature, top_k=None, top_p=None):
    """The words of one row the truncated draw may pick, in numpy (the kernel's rule restated for the tests and CPU doubles): rank
    order by lexsort (y descending, id ascending); top-k keeps the first min(k, V); top-p keeps, within those, the shortest prefix
    whose mass reaches p times their mass.  Masses in float64 from the tempered argument formed in float32, as the kernel forms it.
    -> bool [V]"""
    y = np.asarray(y, dtype=np.float32)
    V = len(y)
    order = np.lexsort((np.arange(V), -y.astype(np.float64)))
    n = V if top_k is None else min(int(top_k), V)
    if temperature == 0:                                   # greedy whatever k and p are
        n = 1
    elif top_p is not None and top_p < 1:
        x = (y - y.max()) * np.float32(1.0 / temperature)
        c = np.cumsum(np.exp(x.astype(np.float64))[order[:n]])
        n = min(int(np.searchsorted(c, top_p * c[-1], side="left")) + 1, n)
    keep = np.zeros(V, dtype=bool)
    keep[order[:n]] = True
    return keep


def check_truncation(top_k, top_p, V):
    """ValueError for a top_k that is not an integer >= 1 or a top_p outside (0, 1].  -> (top_k, top_p) with "off" values (None,
    top_k >= V, top_p >= 1) as None"""
    if top_k is not None:
        if not rowsets.is_int(top_k) or top_k < 1:
            raise ValueError("top_k must be an integer >= 1 (got %r)" % (top_k,))
        top_k = None if top_k >= V else int(top_k)
    if top_p is not None:
        try:
            p = float(top_p)
        except (TypeError, ValueError):
            p = float("nan")
        if isinstance(top_p, bool) or not 0 < p <= 1:
            raise ValueError("top_p must lie in (0, 1] (got %r)" % (top_p,))
        top_p = None if p >= 1 else p
    return top_k, top_p


def check_args(prompts, n_words, temperature, seed, stop_id, V, top_k=None, top_p=None):
    """ValueError for anything the kernels cannot take, before any launch.  -> prompts as int64 arrays"""
    check_truncation(top_k, top_p, V)
    if isinstance(n_words, bool) or not isinstance(n_words, (int, np.integer)) or n_words < 0:
        raise ValueError("n_words must be an integer >= 0 (got %r)" % (n_words,))
    t = float(temperature)
    if not np.isfinite(t) or t < 0:
        raise ValueError("temperature must be finite and >= 0 (got %r)" % (temperature,))
    if not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) <= _M64:
        raise ValueError("seed must be an integer in [0, 2^64) (got %r)" % (seed,))
    out = rowsets.check_prompts([[EOS_ID]] if prompts is None else prompts, V, "generate", "a row needs at least one word to start from")
    if len(out) >= 2 ** 31:
        raise ValueError("too many rows")
    if stop_id is not None:
        check_ids([stop_id], V, "generate (stop_id)")
    return out


def truncate(ids, stop_id):
    """a row's draws up to and including its first ``stop_id`` (all of them without one)"""
    if stop_id is None:
        return ids
    hit = np.nonzero(ids == stop_id)[0]
    return ids[:hit[0] + 1] if len(hit) else ids


class Generator:
    """The device side of a sampling call over a :class:`jlm_amd.model.DeviceModel`."""

    def __init__(self, dev_model):
        self.m = dev_model
        self.torch = dev_model.torch
        self.last_frame_ms = None         # [frames, 4] of the last timed call: LSTM step, T projection, logit GEMMs, draw

    def row_bytes(self, n_prompt, n_words):
        m = self.m
        return (rowsets.ld_logits(m.V) + 4 * m.H + m.ldt) * 4 + n_prompt * 8 + n_words * 12 + 32

    def run(self, prompts, row_id, n_words, temperature, seed, stop_id=None, timed=False, n_live=None, top_k=None, top_p=None):
        """One call over rows already sorted by prompt length (longest first).  row_id [R]: the caller's index of each row.  n_live:
        the chunk's live counts from plan_rows (None: rowsets.live_counts of the prompts).  top_k / top_p as check_truncation
        returns them (None: off).  -> (ids [n_words, R] int32, nll [n_words, R] float64); a stopped row's later positions hold
        -1 / 0."""
        torch, m = self.torch, self.m
        if n_live is None:
            n_live = rowsets.live_counts([len(p) for p in prompts])
        R, P = len(prompts), len(n_live)
        prompt, prev = prompt_arrays(prompts, P)
        dev, i32 = m.device, torch.int32
        s = int(seed) & _M64
        s = s - (1 << 64) if s >= 1 << 63 else s
        with m._ctx():
            rs = rowsets.RowSets(m, R, logits=True)
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
            word = torch.zeros(R, device=dev, dtype=i32)
            done = torch.zeros(R, device=dev, dtype=i32) if stop_id is not None else None
            ids = torch.full((n_words, R), -1, device=dev, dtype=i32)
            nll = torch.zeros((n_words, R), device=dev, dtype=torch.float64)
            args = (m.decode_model(), *rs.state(), rs.logits, rs.ld_logits, rs.rows, up(prev), up(prompt), up(n_live),
                    [int(x) for x in n_live], up(row_id), word, done, -1 if stop_id is None else int(stop_id), float(temperature), s, ids,
                    nll, rs.flags, R, P, int(n_words), bool(timed))
            if top_k is None and top_p is None:
                ms = _ops.backend().generate_frames(*args)
            else:
                ms = _ops.backend().generate_frames_trunc(*args, 0 if top_k is None else int(top_k), 1.0 if top_p is None else float(top_p))
            if timed:
                self.last_frame_ms = ms.numpy()
            rs.check_flags("the draw kernel flagged a logit or log-normaliser that is not finite (flags %d)")
            return ids.cpu().numpy(), nll.cpu().numpy()


def generate(gen, prompts, n_words, temperature=1.0, seed=0, stop_id=None, max_rows=None, top_k=None, top_p=None):
    """LSTM_Model.generate: see there."""
    prompts = check_args(prompts, n_words, temperature, seed, stop_id, gen.m.V, top_k, top_p)
    top_k, top_p = check_truncation(top_k, top_p, gen.m.V)
    lens = [len(p) for p in prompts]
    ids_out = [np.zeros(0, dtype=np.int64) for _ in prompts]
    nll_out = [np.zeros(0, dtype=np.float64) for _ in prompts]
    if n_words == 0 or not prompts:
        return ids_out, nll_out
    if max_rows is None:
        max_rows = rowsets.clamp_rows(MAX_ROWS, GENERATE_BUDGET_BYTES, gen.row_bytes(max(lens), n_words), gen.m.H)
    for ch in plan_rows(lens, max_rows):
        idx = ch["idx"]
        ids, nll = gen.run([prompts[i] for i in idx], idx.astype(np.int32), int(n_words), temperature, seed, stop_id, n_live=ch["n_live"],
                           top_k=top_k, top_p=top_p)
        for j, i in enumerate(idx):
            x = truncate(ids[:, j].astype(np.int64), stop_id)
            ids_out[i] = x
            nll_out[i] = nll[:len(x), j].copy()
    return ids_out, nll_out


def encode_prompt(text, vocab):
    """``--prompt`` as ids: <eos>, then the words through Vocab.w2i (a character model: the characters of the surfaces through
    CharVocab.c2i) with <unk> for anything outside it, as perplexity.encode_lines encodes a line -- without its trailing <eos>.
    -> (ids, number of <unk> fallbacks)"""
    from .perplexity import encode_lines
    if text is None or not text.strip():
        return [EOS_ID], 0
    enc, n_unk = encode_lines([text], vocab)
    return [vocab.t2i["<eos>"]] + enc[0][:-1], n_unk


def render(ids, vocab):
    """the reference's print: ' '.join(x.split('/')[0] ...) over the words (a character model: the characters, joined)"""
    from .data import CharVocab
    if isinstance(vocab, CharVocab):
        return "".join(vocab.i2c.get(int(i), "<unk>") for i in ids)
    return " ".join(vocab.i2w[int(i)].split("/")[0] for i in ids)


def main(argv=None):
    from .data import CharVocab, load_vocab
    ap = argparse.ArgumentParser(description="Sample word sequences from a dumped model on the device (reference decoder/model.py:213-245)")
    _config.add_model_args(ap)
    ap.add_argument("-n", "--rows", type=int, default=1, help="samples to draw")
    ap.add_argument("--words", type=int, default=100, help="words per sample")
    ap.add_argument("--temperature", type=float, default=1.0, help="0 = greedy")
    ap.add_argument("--top-k", type=int, default=None, metavar="N", help="draw from the N most probable words only")
    ap.add_argument("--top-p", type=float, default=None, metavar="P",
                    help="draw from the smallest set of most probable words whose mass reaches P (nucleus sampling; after --top-k)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--prompt", default=None, help='words to continue, "w/r w/r ..." (default: start at <eos>)')
    ap.add_argument("--stop-at-eos", action="store_true", help="end a sample after it draws <eos>")
    ap.add_argument("--show-nll", action="store_true", help="append each sample's total -log p and its word count")
    args = ap.parse_args(argv)
    _cfg, vocab = load_vocab(args)
    from .model import LSTM_Model
    prompt, n_unk = encode_prompt(args.prompt, vocab)
    if n_unk:
        print("prompt: %d word(s) outside the vocabulary read as <unk>" % n_unk, file=sys.stderr)
    model = LSTM_Model(experiment_id=args.experiment_id, comp=args.comp)
    t0 = time.time()
    ids, nll = model.generate([prompt] * args.rows, args.words, temperature=args.temperature, seed=args.seed,
                              stop_id=EOS_ID if args.stop_at_eos else None, top_k=args.top_k, top_p=args.top_p)
    dt = time.time() - t0
    head = render(prompt[1:], vocab)
    sep = "" if isinstance(vocab, CharVocab) or not head else " "
    for x, l in zip(ids, nll):
        line = head + sep + render(x, vocab)
        if args.show_nll:
            line += "\t%.4f\t%d" % (float(l.sum()), len(x))
        print(line)
    n_tok = sum(len(x) for x in ids)
    print("rows: {}  words: {}  words/s: {:.0f}".format(len(ids), n_tok, n_tok / dt if dt > 0 else float("inf")), file=sys.stderr)
    return ids, nll


if __name__ == "__main__":
    main()
