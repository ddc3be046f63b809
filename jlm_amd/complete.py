"""Next-word prediction and beam-search completion on the device: ``LSTM_Model.predict_top``, ``LSTM_Model.complete`` and
``python -m jlm_amd.complete``.

The other question an IME asks its language model is *what comes next?*: the next-word candidates shown after a conversion, and the
few most likely continuations of a phrase.  The reference answers the first with ``find_top_N`` (decoder/model.py:25-26), an argsort
of one host-side distribution, and has no loop for the second.  Here one call is ONE op (``torch.ops.jlm.complete_frames``,
csrc/jlm_decode.hip ``jlm_complete_frames``) over many prompts: per frame the LSTM step, the T projection, the full-vocabulary logits,
``topk_rows_kernel`` (the ``beam_width`` best words of every row, read once) and ``beam_merge_kernel`` (per prompt, the next beam and
its back-pointers; csrc/jlm_topk.hip).  The back-pointers come to the host once per call.

Semantics (pinned by tests/test_complete_cpu.py and tests/test_gpu_complete.py):
  - a prompt starts from the zero state and is consumed as ``generate`` consumes one; frame 0 expands its one distribution, every
    later frame expands each hypothesis the previous frame kept with every word;
  - a hypothesis's score is its summed -log p in f64 (per word: lse - y, lse in f32 expf / f64 sums; -y on self-normalised models);
  - each frame keeps the ``beam_width`` best candidates by (score, the parent's rank in the previous beam, word id), all ascending;
  - with ``stop_id`` a hypothesis ending in it is finished: later frames carry it as one candidate (score unchanged, word -1) that
    ranks by the same key and is never expanded.
Per-row top-``beam_width`` lists are enough: within a row the key orders by nll, then id -- the row kernel's order.

Prompts are right-aligned and sorted longest first (generate's row plan); a prompt's ``beam_width`` rows stay in one call.

Word sets (``predict_top(allowed=)``, ``complete(first_allowed=)``; ``LSTM_Model.predict_reading`` / ``complete_reading`` over a
:class:`jlm_amd.readings.ReadingIndex`): frame 0 selects each prompt's candidates among the words of its set only
(``torch.ops.jlm.complete_frames_masked``, ``topk_rows_masked_kernel``), every later frame is free.  The log-normaliser still runs
over the whole vocabulary, so scores stay -log p under the full distribution, comparable with ``score()``.  A set smaller than the
beam pads frame 0's list with (-1, +inf): such a candidate becomes a finished hypothesis of infinite score that is never expanded,
and hypotheses whose total is not finite are dropped from the result.

A back-off n-gram mixture (``ngram=`` of all four entry points, a :class:`jlm_amd.ngram.NGramMix`): every
selecting frame's rows are patched into the logits of (1 - lam) p_lm + lam q(. | h) before the selection, masked or not
(``torch.ops.jlm.complete_frames_ngram``, csrc/jlm_ngram_mix.hip), h the last two words of the prompt followed by the hypothesis's own,
carried on the device behind every merge.  ``ngram=None`` calls exactly the op it called before.
"""
import argparse
import sys
import time

import numpy as np

from . import config as _config
from . import generate as _gen
from . import ops as _ops
from . import rowsets
from .readings import ReadingIndex
from .rowsets import check_ids, is_int

MAX_BEAM = 64                        # JLM_TOPK_MAX: one lane per rank in the merge, one selection round per rank in the row kernel
MAX_ROWS = _gen.MAX_ROWS
COMPLETE_BUDGET_BYTES = _gen.GENERATE_BUDGET_BYTES
EOS_ID = _gen.EOS_ID


def check_args(prompts, n_words, beam_width, n_best, stop_id, V):
    """ValueError for anything the kernels cannot take, before any launch.  -> (prompts as int64 arrays, n_best)"""
    if not is_int(n_words) or n_words < 1:
        raise ValueError("n_words must be an integer >= 1 (got %r)" % (n_words,))
    if not is_int(beam_width) or not 1 <= beam_width <= min(MAX_BEAM, V):
        raise ValueError("beam_width must be an integer in [1, %d] (got %r)" % (min(MAX_BEAM, V), beam_width))
    if n_best is None:
        n_best = int(beam_width)
    if not is_int(n_best) or not 1 <= n_best <= beam_width:
        raise ValueError("n_best must be an integer in [1, beam_width = %d] (got %r)" % (beam_width, n_best))
    out = rowsets.check_prompts(prompts, V, "complete", "a prompt needs at least one word")
    if stop_id is not None:
        if not is_int(stop_id):
            raise ValueError("stop_id must be an integer word id (got %r)" % (stop_id,))
        check_ids([stop_id], V, "complete (stop_id)")
    return out, int(n_best)


def check_allowed(allowed, n_prompts, V, what):
    """``allowed`` / ``first_allowed``: None, or per prompt None (unrestricted) or word ids.  ValueError before any launch for a wrong
    length or an id outside [0, V).  -> None, or per prompt None or the set's ids (int64, ascending, each once)"""
    if allowed is None:
        return None
    if len(allowed) != n_prompts:
        raise ValueError("%s: one entry per prompt, each None or an array of word ids (%d prompts)" % (what, n_prompts))
    out = []
    for a in allowed:
        if a is None:
            out.append(None)
            continue
        a = np.asarray(a)
        if a.ndim != 1 or (a.size and a.dtype.kind not in "iu"):
            raise ValueError("%s: a word set is a one-dimensional array of integer word ids" % what)
        check_ids(a, V, what)
        out.append(np.unique(a.astype(np.int64)))
    return out


def plan_prompts(lengths, beam_width, max_rows):
    """generate's row plan (rowsets.plan_prompts) cut into chunks of at most max(1, max_rows // beam_width) prompts: a prompt's rows
    never split across calls.  (idx = the caller's prompt of each chunk prompt.)"""
    return rowsets.plan_prompts(lengths, max_rows, beam_width)


# ------------------------------------------------------------------------------------------------- numpy restatements (the tests')
def topk_reference(y, k, self_norm=False):
    """The row kernel restated: the k best of f32 logits ``y`` (one row) by y descending, equal logits lower id first, and their
    nll = lse - y in f64 (self_norm: -y).  -> (ids int64 [k], nll float64 [k])"""
    y = np.asarray(y, dtype=np.float32)
    order = np.lexsort((np.arange(len(y)), -y.astype(np.float64)))[:k]
    yd = y.astype(np.float64)
    if self_norm:
        return order.astype(np.int64), -yd[order]
    m = yd.max()
    lse = m + np.log(np.exp(yd - m).sum())
    return order.astype(np.int64), lse - yd[order]


def topk_masked_reference(y, k, allowed, self_norm=False):
    """The masked row kernel restated: the k best of the ``allowed`` words of f32 logits ``y`` (one row), ranked as topk_reference
    ranks (a NaN logit never ranks), with nll = lse - y where the lse runs over EVERY word of the row (self_norm: -y); fewer than k
    rankable words: padded with id -1 and nll +inf.  -> (ids int64 [k], nll float64 [k])"""
    y = np.asarray(y, dtype=np.float32)
    yd = y.astype(np.float64)
    a = np.unique(np.asarray(allowed, dtype=np.int64).reshape(-1))
    a = a[~np.isnan(yd[a])]
    order = a[np.lexsort((a, -yd[a]))][:k]
    ids = np.full(k, -1, dtype=np.int64)
    nll = np.full(k, np.inf)
    ids[:len(order)] = order
    if self_norm:
        nll[:len(order)] = -yd[order]
    else:
        m = yd.max()
        nll[:len(order)] = (m + np.log(np.exp(yd - m).sum())) - yd[order]
    return ids, nll


def merge_reference(cand_ids, cand_nll, score, finished, beam, n_prompts, first, stop_id=-1):
    """The merge restated: per prompt, every candidate of its rows' lists (a finished parent: one carry, word -1, nll 0), sorted by
    (score, parent rank, word), the first ``beam`` kept.  cand_* [rows, beam]; score / finished [n_prompts * beam] (ignored when
    ``first``).  -> dict of [n_prompts * beam] arrays: word, prev, score, finished, bp_parent, bp_word, bp_nll"""
    B = beam
    R = n_prompts * B
    out = dict(word=np.zeros(R, np.int32), prev=np.zeros(R, np.int32), score=np.zeros(R), finished=np.zeros(R, np.int32),
               bp_parent=np.zeros(R, np.int32), bp_word=np.zeros(R, np.int32), bp_nll=np.zeros(R))
    for p in range(n_prompts):
        cs, cp, cw, cn = [], [], [], []
        for j in range(1 if first else B):
            src = p if first else p * B + j
            ps = 0.0 if first else float(score[src])
            if not first and finished[src]:
                cs.append(ps); cp.append(j); cw.append(-1); cn.append(0.0)
                continue
            for i in range(B):
                cs.append(ps + float(cand_nll[src, i])); cp.append(j); cw.append(int(cand_ids[src, i])); cn.append(float(cand_nll[src, i]))
        cs, cp, cw, cn = np.array(cs), np.array(cp), np.array(cw), np.array(cn)
        keep = np.lexsort((cw, cp, cs))[:B]
        for i, c in enumerate(keep):
            q = p * B + i
            w = int(cw[c])
            out["score"][q] = cs[c]
            out["finished"][q] = int(w < 0 or (stop_id is not None and stop_id >= 0 and w == stop_id))
            out["word"][q] = w if w >= 0 else max(int(stop_id if stop_id is not None else 0), 0)
            out["prev"][q] = p if first else p * B + int(cp[c])
            out["bp_parent"][q] = cp[c]
            out["bp_word"][q] = w
            out["bp_nll"][q] = cn[c]
    return out


def backtrace(bp_parent, bp_word, bp_nll, score, p, beam, n_best, stop_id=None):
    """Prompt p's ``n_best`` best hypotheses from back-pointers [n_words, rows] (rank i of prompt p at row p * beam + i) and the final
    scores [rows]: walked from the last frame to the first, carries (word -1) dropped, cut after ``stop_id``.
    -> list of (ids int64, nll float64, total), best first"""
    out = []
    N = bp_parent.shape[0]
    for i in range(n_best):
        j, ws, ns = i, [], []
        for k in range(N - 1, -1, -1):
            q = p * beam + j
            if bp_word[k, q] >= 0:
                ws.append(int(bp_word[k, q]))
                ns.append(float(bp_nll[k, q]))
            j = int(bp_parent[k, q])
        ids = _gen.truncate(np.array(ws[::-1], dtype=np.int64), stop_id)
        out.append((ids, np.array(ns[::-1][:len(ids)], dtype=np.float64), float(score[p * beam + i])))
    return out


class Completer:
    """The device side of a beam-search call over a :class:`jlm_amd.model.DeviceModel`."""

    def __init__(self, dev_model):
        self.m = dev_model
        self.torch = dev_model.torch
        self.last_frame_ms = None         # [frames, 5] of the last timed call: LSTM step, T projection, logit GEMMs, selection, merge

    def row_bytes(self, n_prompt, n_words, beam, ngram=False):
        """the bytes a row of a call takes; ``ngram``: with its two history entries (jlm_amd.ngram_mix.BeamHist)"""
        m = self.m
        return (rowsets.ld_logits(m.V) + 4 * m.H + m.ldt) * 4 + beam * 12 + n_words * 16 + n_prompt * 8 + 48 + (16 if ngram else 0)

    def run(self, prompts, n_words, beam, stop_id=None, timed=False, n_live=None, first_sets=None, ngram=None):
        """One call over prompts already sorted by length (longest first).  n_live: the chunk's live counts from plan_prompts (None:
        rowsets.live_counts of the prompts).  first_sets: None, or per prompt None or the word ids its first word is chosen among
        (the masked op; None leaves the call exactly what it was).  ngram: None, or a checked :class:`jlm_amd.ngram.NGramMix` -- the
        op is then ``complete_frames_ngram``, masked or not: every selecting frame's rows are patched into the mixture of the
        hypothesis's own last two words before the selection (jlm_amd/ngram_mix.py).  -> (bp_parent, bp_word [n_words, R] int32, bp_nll [n_words, R]
        float64, score [R] float64), R = len(prompts) * beam, rank i of prompt p at row p * beam + i."""
        torch, m = self.torch, self.m
        if n_live is None:
            n_live = rowsets.live_counts([len(p) for p in prompts])
        NP, B, P = len(prompts), int(beam), len(n_live)
        R = NP * B
        prompt, prev = rowsets.prompt_arrays(prompts, P)
        dev, i32, f64 = m.device, torch.int32, torch.float64
        with m._ctx():
            rs = rowsets.RowSets(m, R, logits=True)
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
            cand_ids = torch.empty((R, B), device=dev, dtype=i32)
            cand_nll = torch.empty((R, B), device=dev, dtype=f64)
            word = torch.zeros(R, device=dev, dtype=i32)
            prev_row = torch.zeros(R, device=dev, dtype=i32)
            score = torch.zeros(R, device=dev, dtype=f64)
            finished = torch.zeros(R, device=dev, dtype=i32)
            bp_parent = torch.zeros((n_words, R), device=dev, dtype=i32)
            bp_word = torch.full((n_words, R), -1, device=dev, dtype=i32)
            bp_nll = torch.zeros((n_words, R), device=dev, dtype=f64)
            args = (m.decode_model(), *rs.state(), rs.logits, rs.ld_logits, rs.rows, up(prev), up(prompt), up(n_live),
                    [int(x) for x in n_live], cand_ids, cand_nll, word, prev_row, score, finished, -1 if stop_id is None else int(stop_id),
                    bp_parent, bp_word, bp_nll, rs.flags, NP, B, P, int(n_words), bool(timed))
            mask_args = (None, 0, 0, [])
            if first_sets is not None:
                restricted = [p for p in range(NP) if first_sets[p] is not None]
                mask, index = ReadingIndex.mask([first_sets[p] for p in restricted], m.V)
                prompt_set = [-1] * NP
                for p, s in zip(restricted, index):
                    prompt_set[p] = int(s)
                mask_args = (torch.from_numpy(mask.view(np.int32)).to(dev), mask.shape[1], mask.shape[0], prompt_set)
            if ngram is not None:
                from .ngram_mix import BeamHist
                bh = BeamHist(m, ngram, prompts, R)
                ms = _ops.backend().complete_frames_ngram(*args, *mask_args, *bh.op_args())
            elif first_sets is None:
                ms = _ops.backend().complete_frames(*args)
            else:
                ms = _ops.backend().complete_frames_masked(*args, *mask_args)
            if timed:
                self.last_frame_ms = ms.numpy()
            if ngram is not None:
                bh.check()
            rs.check_flags("topk_rows_kernel flagged a logit or log-normaliser that is not finite (flags %d)")
            return bp_parent.cpu().numpy(), bp_word.cpu().numpy(), bp_nll.cpu().numpy(), score.cpu().numpy()


def complete(comp, prompts, n_words, beam_width=10, n_best=None, stop_id=None, max_rows=None, first_allowed=None, ngram=None):
    """LSTM_Model.complete: see there."""
    prompts, n_best = check_args(prompts, n_words, beam_width, n_best, stop_id, comp.m.V)
    if ngram is not None:
        from .ngram import check_mix_rows
        check_mix_rows(ngram, comp.m.V)
    # a self-normalised model under the mixture: the kernels score -y', and -log p of a word is -y' - log1p(-lam)
    shift = -np.log1p(-float(np.float32(ngram.lam))) if ngram is not None and comp.m.self_norm else 0.0
    sets = check_allowed(first_allowed, len(prompts), comp.m.V, "complete (first_allowed)")
    out = [None] * len(prompts)
    if not prompts:
        return out
    run = list(range(len(prompts)))                      # the prompts that reach the device: an empty set has no completion
    if sets is not None:
        run = [i for i in run if sets[i] is None or len(sets[i])]
        for i in range(len(prompts)):
            out[i] = []
        if not run:
            return out
    lens = [len(prompts[i]) for i in run]
    if max_rows is None:
        max_rows = rowsets.clamp_rows(MAX_ROWS, COMPLETE_BUDGET_BYTES, comp.row_bytes(max(lens), n_words, beam_width, ngram is not None), comp.m.H)
    for ch in plan_prompts(lens, beam_width, max_rows):
        idx = [run[j] for j in ch["idx"]]
        bp_parent, bp_word, bp_nll, score = comp.run([prompts[i] for i in idx], int(n_words), int(beam_width), stop_id, n_live=ch["n_live"],
                                                     first_sets=None if sets is None else [sets[i] for i in idx], ngram=ngram)
        for j, i in enumerate(idx):
            out[i] = backtrace(bp_parent, bp_word, bp_nll, score, j, int(beam_width), n_best, stop_id)
            if shift:
                out[i] = [(ids, nll + shift, total + shift * len(ids)) for ids, nll, total in out[i]]     # (a carry adds no word)
            if sets is not None:                         # a set smaller than the beam: the padding's hypotheses have infinite totals
                out[i] = [h for h in out[i] if np.isfinite(h[2])]
    return out


def predict_top(comp, contexts, n=10, max_rows=None, allowed=None, ngram=None):
    """LSTM_Model.predict_top: see there.  Frame 0 of complete(contexts, 1, beam_width=n)."""
    res = complete(comp, contexts, 1, beam_width=n, max_rows=max_rows, first_allowed=allowed, ngram=ngram)
    return [(np.array([h[0][0] for h in r], dtype=np.int64), -np.array([h[1][0] for h in r], dtype=np.float64)) for r in res]


def build_parser():
    ap = argparse.ArgumentParser(description="Predict next words or complete phrases by beam search on the device "
                                             "(reference decoder/model.py:25-26 find_top_N)")
    _config.add_model_args(ap)
    src = ap.add_mutually_exclusive_group()
    src.add_argument("--prompt", default=None, help='words to continue, "w/r w/r ..." (default: start at <eos>)')
    src.add_argument("--file", default=None, help="one prompt per line")
    ap.add_argument("--words", type=int, default=3, help="words per completion")
    ap.add_argument("-b", "--beam", type=int, default=10, help="beam width (<= 64)")
    ap.add_argument("--n-best", type=int, default=None, help="completions to print per prompt (default: the beam width)")
    ap.add_argument("--top", type=int, default=None, metavar="N", help="next-word mode: the N most probable next words")
    ap.add_argument("--stop-at-eos", action="store_true", help="end a completion after <eos>")
    ap.add_argument("--reading", default=None, metavar="KANA",
                    help="only words whose reading starts with KANA (hiragana or katakana): with --top the next words, else the first "
                         "word of every completion")
    ap.add_argument("--exact", action="store_true", help="with --reading: the reading equals KANA")
    ap.add_argument("--convert", default=None, metavar="KANA",
                    help="convert KANA whose last word may be unfinished (Decoder.decode_predict): prints the conversions and the "
                         "predictions of the last word; --prompt is the left context, -b the beam, --n-best the lists' length")
    ap.add_argument("--candidates", default=None, metavar="KANA",
                    help="convert KANA and list, for every segment of the best conversion, the words that could stand there, best first "
                         "(Decoder.decode_candidates); --prompt is the left context, -b the beam")
    ap.add_argument("--ngram", default=None, metavar="FILE",
                    help="mix a back-off n-gram model (ARPA text, python -m jlm_amd.ngram) into every distribution the words are chosen "
                         "from: with --top the next words, else every word of every completion; with --reading too")
    ap.add_argument("--ngram-lam", type=float, default=None, dest="ngram_lam", help="--ngram: the n-gram model's weight, in (0, 1)")
    ap.add_argument("--ngram-order", type=int, default=3, dest="ngram_order", help="--ngram: the order FILE is read at (1, 2 or 3)")
    ap.add_argument("--n-cand", type=int, default=10, help="with --candidates: words per segment (<= 64)")
    ap.add_argument("--lookahead", type=int, default=None, metavar="J",
                    help="with --candidates: words of the path re-scored behind a substitute (default: all of them)")
    return ap


def candidates_main(args, vocab, prompts):
    """--candidates: one (conversions, segments) pair per prompt, printed as the best conversion and one list per segment"""
    from .decoder import Decoder
    dec = Decoder(experiment_id=args.experiment_id, comp=args.comp)
    t0 = time.time()
    res = dec.decode_candidates_batch([args.candidates] * len(prompts), topN=1, beam_width=args.beam, n_cand=args.n_cand,
                                      lookahead=args.lookahead, context=[list(p[1:]) for p in prompts])
    dt = time.time() - t0
    for b, (p, (conv, segs)) in enumerate(zip(prompts, res)):
        if b:
            print()
        head = _gen.render(p[1:], vocab)
        print("conversion%s:" % (" after " + head if head else ""))
        print("%s\t%.4f" % (" ".join(w.split("/")[0] for w in conv[0][1]), conv[0][0]))
        for start, length, cands in segs:
            print("segment %d+%d %s:" % (start, length, args.candidates[start:start + length]))
            for score, word in cands:
                print("%s\t%.4f" % (word.split("/")[0], score))
    n_out = sum(len(c) for _conv, segs in res for _s, _l, c in segs)
    print("inputs: {}  segments: {}  candidates/s: {:.0f}".format(len(prompts), sum(len(sg) for _c, sg in res),
                                                                  n_out / dt if dt > 0 else float("inf")), file=sys.stderr)
    return res


def convert_main(args, vocab, prompts):
    """--convert: one (conversions, predictions) pair per prompt, printed as two lists"""
    from .decoder import Decoder
    dec = Decoder(experiment_id=args.experiment_id, comp=args.comp)
    n = 10 if args.n_best is None else args.n_best
    t0 = time.time()
    res = dec.decode_predict_batch([args.convert] * len(prompts), topN=n, beam_width=args.beam, context=[list(p[1:]) for p in prompts])
    dt = time.time() - t0
    for b, (p, (conv, pred)) in enumerate(zip(prompts, res)):
        if b:
            print()
        head = _gen.render(p[1:], vocab)
        for title, lst in (("conversions", conv), ("predictions", pred)):
            print("%s%s:" % (title, " after " + head if head else ""))
            for score, words in lst:
                print("%s\t%.4f" % (" ".join(w.split("/")[0] for w in words), score))
    n_out = sum(len(c) + len(q) for c, q in res)
    print("inputs: {}  lists: {}  paths/s: {:.0f}".format(len(prompts), 2 * len(prompts), n_out / dt if dt > 0 else float("inf")),
          file=sys.stderr)
    return res


def main(argv=None):
    from .data import CharVocab, load_vocab
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.exact and args.reading is None:
        ap.error("--exact needs --reading")
    if args.ngram is not None and (args.ngram_lam is None or not 0.0 < args.ngram_lam < 1.0 or args.ngram_order not in (1, 2, 3)):
        ap.error("--ngram needs --ngram-lam in (0, 1); --ngram-order is 1, 2 or 3")
    if args.ngram is None and args.ngram_lam is not None:
        ap.error("--ngram-lam goes with --ngram")
    if args.ngram is not None and (args.convert is not None or args.candidates is not None):
        ap.error("--ngram goes with --top and with completions, not with --convert / --candidates")
    _cfg, vocab = load_vocab(args)
    if args.reading is not None and isinstance(vocab, CharVocab):
        ap.error("--reading needs a word model: a character model's softmax is not over words")
    if args.ngram is not None and isinstance(vocab, CharVocab):
        ap.error("--ngram needs a word model: the table is over words")
    from .model import LSTM_Model
    if args.file:
        with open(args.file, encoding="utf-8") as f:
            texts = [l.rstrip("\n") for l in f if l.strip()]
    else:
        texts = [args.prompt]
    prompts, n_unk = [], 0
    for t in texts:
        p, u = _gen.encode_prompt(t, vocab)
        prompts.append(p)
        n_unk += u
    if n_unk:
        print("prompts: %d word(s) outside the vocabulary read as <unk>" % n_unk, file=sys.stderr)
    if args.candidates is not None:
        if args.convert is not None or args.reading is not None or args.top is not None or isinstance(vocab, CharVocab):
            ap.error("--candidates is a mode of its own (no --convert / --reading / --top), on a word model")
        return candidates_main(args, vocab, prompts)
    if args.convert is not None:
        if args.reading is not None or args.top is not None or isinstance(vocab, CharVocab):
            ap.error("--convert is a mode of its own (no --reading / --top), on a word model")
        return convert_main(args, vocab, prompts)
    model = LSTM_Model(experiment_id=args.experiment_id, comp=args.comp)
    sep = "" if isinstance(vocab, CharVocab) else " "
    t0 = time.time()
    readings = None if args.reading is None else [args.reading] * len(prompts)
    mix = None
    if args.ngram is not None:
        import os
        from .ngram import NGramMix, NGramTable
        path = args.ngram if os.path.exists(args.ngram) else os.path.join(_config.data_path, args.ngram)
        mix = NGramMix(NGramTable.from_srilm(path, vocab.t2i, args.ngram_order), args.ngram_lam)
    if args.top is not None:
        res = (model.predict_top(prompts, n=args.top, ngram=mix) if readings is None else
               model.predict_reading(prompts, readings, n=args.top, exact=args.exact, ngram=mix))
        dt = time.time() - t0
        for b, (p, (ids, logp)) in enumerate(zip(prompts, res)):
            if b:
                print()
            head = _gen.render(p[1:], vocab)
            for w, lp in zip(ids, logp):
                print("%s%s%s\t%.4f" % (head, sep if head else "", _gen.render([w], vocab), -lp))
        n_out = sum(len(r[0]) for r in res)
    else:
        kw = dict(beam_width=args.beam, n_best=args.n_best, stop_id=EOS_ID if args.stop_at_eos else None, ngram=mix)
        res = (model.complete(prompts, args.words, **kw) if readings is None else
               model.complete_reading(prompts, readings, args.words, exact=args.exact, **kw))
        dt = time.time() - t0
        for b, (p, hyps) in enumerate(zip(prompts, res)):
            if b:
                print()
            head = _gen.render(p[1:], vocab)
            for ids, _nll, total in hyps:
                tail = _gen.render(ids, vocab)
                print("%s%s%s\t%.4f" % (head, sep if head and tail else "", tail, total))
        n_out = sum(len(h[0]) for r in res for h in r)
    print("prompts: {}  words: {}  words/s: {:.0f}".format(len(prompts), n_out, n_out / dt if dt > 0 else float("inf")),
          file=sys.stderr)
    return res


if __name__ == "__main__":
    main()
