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
"""
import argparse
import sys
import time

import numpy as np

from . import config as _config
from . import generate as _gen
from . import ops as _ops
from . import rowsets
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

    def row_bytes(self, n_prompt, n_words, beam):
        m = self.m
        return (rowsets.ld_logits(m.V) + 4 * m.H + m.ldt) * 4 + beam * 12 + n_words * 16 + n_prompt * 8 + 48

    def run(self, prompts, n_words, beam, stop_id=None, timed=False, n_live=None):
        """One call over prompts already sorted by length (longest first).  n_live: the chunk's live counts from plan_prompts (None:
        rowsets.live_counts of the prompts).  -> (bp_parent, bp_word [n_words, R] int32, bp_nll [n_words, R] float64, score [R]
        float64), R = len(prompts) * beam, rank i of prompt p at row p * beam + i."""
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
            ms = _ops.backend().complete_frames(m.decode_model(), *rs.state(), rs.logits, rs.ld_logits, rs.rows, up(prev), up(prompt),
                                                up(n_live), [int(x) for x in n_live], cand_ids, cand_nll, word, prev_row, score,
                                                finished, -1 if stop_id is None else int(stop_id), bp_parent, bp_word, bp_nll, rs.flags,
                                                NP, B, P, int(n_words), bool(timed))
            if timed:
                self.last_frame_ms = ms.numpy()
            rs.check_flags("topk_rows_kernel flagged a logit or log-normaliser that is not finite (flags %d)")
            return bp_parent.cpu().numpy(), bp_word.cpu().numpy(), bp_nll.cpu().numpy(), score.cpu().numpy()


def complete(comp, prompts, n_words, beam_width=10, n_best=None, stop_id=None, max_rows=None):
    """LSTM_Model.complete: see there."""
    prompts, n_best = check_args(prompts, n_words, beam_width, n_best, stop_id, comp.m.V)
    out = [None] * len(prompts)
    if not prompts:
        return out
    lens = [len(p) for p in prompts]
    if max_rows is None:
        max_rows = rowsets.clamp_rows(MAX_ROWS, COMPLETE_BUDGET_BYTES, comp.row_bytes(max(lens), n_words, beam_width), comp.m.H)
    for ch in plan_prompts(lens, beam_width, max_rows):
        idx = ch["idx"]
        bp_parent, bp_word, bp_nll, score = comp.run([prompts[i] for i in idx], int(n_words), int(beam_width), stop_id, n_live=ch["n_live"])
        for j, i in enumerate(idx):
            out[i] = backtrace(bp_parent, bp_word, bp_nll, score, j, int(beam_width), n_best, stop_id)
    return out


def predict_top(comp, contexts, n=10, max_rows=None):
    """LSTM_Model.predict_top: see there.  Frame 0 of complete(contexts, 1, beam_width=n)."""
    res = complete(comp, contexts, 1, beam_width=n, max_rows=max_rows)
    return [(np.array([h[0][0] for h in r], dtype=np.int64), -np.array([h[1][0] for h in r], dtype=np.float64)) for r in res]


def main(argv=None):
    from .data import CharVocab, load_vocab
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
    args = ap.parse_args(argv)
    _cfg, vocab = load_vocab(args)
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
    model = LSTM_Model(experiment_id=args.experiment_id, comp=args.comp)
    sep = "" if isinstance(vocab, CharVocab) else " "
    t0 = time.time()
    if args.top is not None:
        res = model.predict_top(prompts, n=args.top)
        dt = time.time() - t0
        for b, (p, (ids, logp)) in enumerate(zip(prompts, res)):
            if b:
                print()
            head = _gen.render(p[1:], vocab)
            for w, lp in zip(ids, logp):
                print("%s%s%s\t%.4f" % (head, sep if head else "", _gen.render([w], vocab), -lp))
        n_out = sum(len(r[0]) for r in res)
    else:
        res = model.complete(prompts, args.words, beam_width=args.beam, n_best=args.n_best,
                             stop_id=EOS_ID if args.stop_at_eos else None)
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
