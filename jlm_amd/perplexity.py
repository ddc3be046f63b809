"""Test perplexity of a dumped model on the device: ``python -m jlm_amd.perplexity``.

The reference reports it at the end of training (train/train.py:101-102: ``Test perplexity: ...`` from run_epoch over the encoded
data/test.txt, train/model.py:262-297).  Here the same number comes from the dumped weights, scored by LSTM_Model.score /
score_streams (jlm_amd/score.py):

  --mode stream    the reference's convention: the encoded file as one id stream, cut by corpus_iterator (train/utils.py:17-31;
                   the tail that does not fill a row or a chunk is dropped) into ``batch_size`` streams of ``num_steps`` chunks, the
                   LSTM state carried from chunk to chunk.  Perplexity = exp(mean -log p), what run_epoch returns.
  --mode sentence  every line on its own, from the zero state: start = <eos>, targets = the line's words + <eos>.
                   Perplexity = exp(sum -log p / number of tokens).

Encoding follows Corpus.encode_corpus (train/data.py:54-70): words through Vocab.w2i with <unk> for anything outside it and <eos>
after every line; a character model (config char_rnn) reads the characters of the surfaces through CharVocab.c2i instead.

  --ranks          after the perplexity line, one line on how good the model's candidate lists are over the same tokens, from
                   LSTM_Model.rank / rank_streams (jlm_amd/rank.py): top-k accuracy (--top), mean reciprocal rank, keystroke
                   savings of a candidate list of --list words, and the position of the word among its homophones.  A character
                   model reports the first two only.  Without --ranks nothing of this runs.
  --cache N        stream mode: also score with a continuous cache of the last N (hidden state, next word) pairs of every stream
                   (jlm_amd/cache.py) at --theta and --lam, in ONE pass -- LSTM_Model.score_streams_cached returns the plain -log p
                   as well -- and print the cached perplexity after the plain one.  --tune-cache FILE sweeps --thetas and --lams on
                   FILE, the dev set, prints the grid's best pair and reports the test perplexity at that pair.  Without --cache the
                   output is what it was.  With --ranks as well (N <= 4096), a second --ranks line "with cache" over the same tokens,
                   at the theta and lam the cached perplexity is reported at (LSTM_Model.rank_streams_cached).  With --ngram FILE
                   as well, a --ranks line "with n-gram" at the lambda the mixture's perplexity is reported at (--ngram-lam, or
                   --tune-ngram's pick): LSTM_Model.rank_streams_ngram patches every step's logits on the device.
  --dynamic        stream mode: after the static line, the dynamically evaluated perplexity (jlm_amd/dyneval.py): the stream read in
                   chunks of -b (default 1) x --de-steps tokens, each scored and then learnt from by --de-rule at --de-lr and --de-lam.
                   Rule rms takes its gradient statistics over --de-stat-chunks chunks of data/train.txt.  --tune-dynamic FILE sweeps
                   --de-lrs x --de-lams on FILE, the dev set, and reports the test perplexity at the best pair.  Not with --cache,
                   --ranks or --mode sentence.  Without --dynamic the output is what it was.
  --memory MEM     stream mode: also score against the memory of hidden states saved in MEM (python -m jlm_amd.memory; jlm_amd/memory.py,
                   DESIGN.md section 28) at --mem-theta and --mem-lam, in ONE pass -- LSTM_Model.score_streams_memory returns the plain
                   -log p as well -- and print the perplexity under the memory after the plain one.  --tune-memory DEV sweeps --thetas
                   and --lams on DEV and reports the test perplexity at the grid's best pair.  Not with --cache, --dynamic or --ngram.
                   Without --memory the output is what it was.  With --ranks and --mem-k K as well, a second --ranks line "with memory"
                   over the same tokens, from LSTM_Model.rank_streams_memory at the K nearest entries, the theta and the lam the
                   memory's perplexity is reported at; without --mem-k nothing of this runs.
"""
import argparse
import os
import time

import numpy as np

from . import config as _config
from .data import CharVocab, load_vocab


def encode_lines(lines, vocab):
    """-> (one id list per line, ending in <eos>; number of <unk> fallbacks).  train/data.py:60-69."""
    out, n_unk = [], 0
    table, unk, eos = vocab.t2i, vocab.t2i["<unk>"], vocab.t2i["<eos>"]
    for line in lines:
        words = line.strip().split(" ")
        if isinstance(vocab, CharVocab):
            words = "".join([word.split("/")[0] for word in words])
        ids = []
        for x in words:
            i = table.get(x)
            if i is None:
                i, n_unk = unk, n_unk + 1
            ids.append(i)
        out.append(ids + [eos])
    return out, n_unk


def read_lines(path, n=0):
    with open(path, "r", encoding="utf-8") as f:
        lines = f.readlines()
    return lines[:n] if n else lines


def sentence_perplexity(model, sents, eos):
    """-> (perplexity, total nll, number of tokens)"""
    nll = model.score(sents, eos, per_token=False)
    n_tok = sum(len(s) for s in sents)
    total = float(np.sum(nll))
    return float(np.exp(total / max(n_tok, 1))), total, n_tok


def stream_perplexity(model, stream, batch_size, num_steps):
    """-> (perplexity, total nll, number of tokens): run_epoch's exp(mean -log p) over the corpus_iterator chunks, state carried"""
    from .score import stream_layout
    x, y = stream_layout(stream, batch_size, num_steps)
    h = c = None
    total, n_tok = 0.0, 0
    for i in range(x.shape[1] // num_steps):
        cols = slice(i * num_steps, (i + 1) * num_steps)
        nll, h, c = model.score_streams(x[:, cols], y[:, cols], h, c)
        total += float(nll.sum())
        n_tok += nll.size
    return float(np.exp(total / n_tok)), total, n_tok


def stream_ngram_scores(model, stream, batch_size, num_steps, table):
    """-> (nll, logq), float64 arrays over the tokens stream_perplexity scores: the model's -log p (score_streams) and the n-gram
    model's q(token | the words before it in its row of the layout) from NGramTable.logq -- what the mixture's perplexity is made of,
    on the host; no kernel beside score_streams' runs"""
    from .score import stream_layout
    x, y = stream_layout(stream, batch_size, num_steps)
    h = c = None
    T = (x.shape[1] // num_steps) * num_steps
    nll = np.zeros((x.shape[0], T))
    for i in range(T // num_steps):
        cols = slice(i * num_steps, (i + 1) * num_steps)
        part, h, c = model.score_streams(x[:, cols], y[:, cols], h, c)
        nll[:, cols] = np.asarray(part, dtype=np.float64)
    logq = np.array([[table.logq(x[r, max(0, t - 1):t + 1], y[r, t]) for t in range(T)] for r in range(x.shape[0])], dtype=np.float64)
    return nll.reshape(-1), logq.reshape(-1)


def ngram_mixture_perplexity(nll, logq, lam):
    """exp(mean -log((1 - lam) p_lm + lam p_ng)) in float64 (jlm_amd.ngram.mixture_nll)"""
    from .ngram import mixture_nll
    return float(np.exp(mixture_nll(nll, logq, lam).mean()))


def stream_cached_scores(model, stream, batch_size, num_steps, spec):
    """-> the :class:`jlm_amd.cache.CachedScores` of every corpus_iterator chunk, state and cache carried, as stream_perplexity"""
    from .score import stream_layout
    x, y = stream_layout(stream, batch_size, num_steps)
    h = c = state = None
    out = []
    for i in range(x.shape[1] // num_steps):
        cols = slice(i * num_steps, (i + 1) * num_steps)
        res = model.score_streams_cached(x[:, cols], y[:, cols], spec, h, c, state)
        h, c, state = res.h, res.c, res.state
        out.append(res)
    return out


def cached_perplexity(parts, lam, theta_index=0):
    """-> (plain perplexity, cached perplexity, number of tokens) of a list of CachedScores; the plain one is stream_perplexity's sum"""
    total = mixed = 0.0
    n_tok = 0
    for p in parts:
        total += float(p.nll_lm.sum())
        mixed += float(p.nll(lam, theta_index).sum())
        n_tok += p.nll_lm.size
    return float(np.exp(total / n_tok)), float(np.exp(mixed / n_tok)), n_tok


def stream_memory_scores(model, stream, batch_size, num_steps, memory, spec):
    """-> the :class:`jlm_amd.memory.MemoryScores` of every corpus_iterator chunk, state carried, as stream_perplexity"""
    from .score import stream_layout
    x, y = stream_layout(stream, batch_size, num_steps)
    h = c = None
    out = []
    for i in range(x.shape[1] // num_steps):
        cols = slice(i * num_steps, (i + 1) * num_steps)
        res = model.score_streams_memory(x[:, cols], y[:, cols], memory, spec, h, c)
        h, c = res.h, res.c
        out.append(res)
    return out


def _floats(text, what, ap):
    try:
        return [float(x) for x in text.split(",") if x.strip()]
    except ValueError:
        ap.error("%s takes comma-separated numbers" % what)


def sentence_ranks(model, sents, eos, readings, max_prefix):
    """-> (ranks [tokens, columns], the targets [tokens]) of every line on its own, as sentence_perplexity scores them"""
    ranks = model.rank(sents, eos, readings=readings, max_prefix=max_prefix)
    width = ranks[0].shape[1] if ranks else 1
    return (np.concatenate(ranks) if ranks else np.zeros((0, width), dtype=np.int32)), np.array([t for s in sents for t in s], dtype=np.int64)


def stream_ranks(model, stream, batch_size, num_steps, readings, max_prefix, spec=None, ngram=None, memory=None):
    """-> (ranks [tokens, columns], the targets [tokens]) over the corpus_iterator chunks, state carried, as stream_perplexity;
    ``spec``: a CacheSpec -- the ranks under the continuous cache (LSTM_Model.rank_streams_cached), the cache carried too; ``ngram``:
    an NGramMix -- the ranks under the n-gram mixture (LSTM_Model.rank_streams_ngram), the streams' last two words carried too; a row's
    first token has the history of its one input word, exactly as stream_ngram_scores gives it to the mixture's perplexity;
    ``memory``: a MemoryMix -- the ranks under the memory's K nearest entries (LSTM_Model.rank_streams_memory)"""
    from .score import stream_layout
    x, y = stream_layout(stream, batch_size, num_steps)
    h = c = state = tail = None
    out = []
    for i in range(x.shape[1] // num_steps):
        cols = slice(i * num_steps, (i + 1) * num_steps)
        if ngram is not None:
            res = model.rank_streams_ngram(x[:, cols], y[:, cols], ngram, h, c, tail, readings=readings, max_prefix=max_prefix)
            r, h, c, tail = res.ranks, res.h, res.c, res.tail
        elif memory is not None:
            res = model.rank_streams_memory(x[:, cols], y[:, cols], memory, h, c, readings=readings, max_prefix=max_prefix)
            r, h, c = res.ranks, res.h, res.c
        elif spec is None:
            r, h, c = model.rank_streams(x[:, cols], y[:, cols], h, c, readings=readings, max_prefix=max_prefix)
        else:
            res = model.rank_streams_cached(x[:, cols], y[:, cols], spec, h, c, state, readings=readings, max_prefix=max_prefix)
            r, h, c, state = res.ranks, res.h, res.c, res.state
        out.append(r)
    ranks = np.concatenate(out, axis=1)
    return ranks.reshape(-1, ranks.shape[-1]), y.reshape(-1).astype(np.int64)


def ranks_line(ranks, targets, index, tops, list_size):
    """the --ranks line: top-k accuracy and MRR over every token; with a reading index also keystroke savings and the homophone
    position over the tokens that have a reading"""
    from . import rank as _rank
    acc = _rank.topk_accuracy(ranks, tops)
    parts = ["top-{}: {:.4f}".format(k, acc[k]) for k in tops] + ["MRR: {:.4f}".format(_rank.mrr(ranks))]
    if index is not None:
        ks = _rank.keystrokes(ranks, _rank.reading_lengths(index)[targets], list_size)
        hp = _rank.homophone_position(ranks)
        parts += ["keystroke savings (list {}): {:.4f}".format(list_size, ks["savings"]),
                  "homophone position: {:.3f} (first: {:.4f})".format(hp["mean"], hp["first"]),
                  "tokens: {} ranked, {} with a reading, {} without".format(len(ranks), ks["tokens"], ks["excluded"])]
    else:
        parts.append("tokens: {} ranked".format(len(ranks)))
    return "  ".join(parts)


def main(argv=None, de_stepper=None):
    """``de_stepper``: the ``stepper`` of ``jlm_amd.dyneval.dynamic_perplexity`` for the --dynamic figures (tests: "reference", the
    float64 stepper, which also gives the static line, from a pass at zero rates, so that nothing needs the device)"""
    ap = argparse.ArgumentParser(description="Test perplexity of a dumped model on the device (reference train/train.py:101-102)")
    _config.add_model_args(ap)
    ap.add_argument("--file", default=None, help="text to score, one sentence per line (default: <root>/data/test.txt)")
    ap.add_argument("--mode", choices=("sentence", "stream"), default="stream")
    ap.add_argument("-b", "--batch_size", type=int, default=None, help="stream mode: parallel streams (default: the config's, else 64)")
    ap.add_argument("--num_steps", type=int, default=20, help="stream mode: steps per chunk")
    ap.add_argument("-es", type=int, default=0, help="score the first N lines only (0 = all)")
    ap.add_argument("--ranks", action="store_true", help="also report top-k accuracy, MRR, keystroke savings and homophone position")
    ap.add_argument("--top", default="1,5,10", help="--ranks: the k of top-k accuracy, comma-separated")
    ap.add_argument("--list", type=int, default=5, dest="list_size", help="--ranks: words in the candidate list of the keystroke figure")
    ap.add_argument("--max_prefix", type=int, default=8, help="--ranks: typed kana up to which a word is looked for in the list")
    ap.add_argument("--cache", type=int, default=0, metavar="N", help="stream mode: also report the perplexity with a continuous cache of N entries")
    ap.add_argument("--theta", type=float, default=0.3, help="--cache: the flatness of the cache distribution")
    ap.add_argument("--lam", type=float, default=0.1, help="--cache: the weight of the cache in the mixture")
    ap.add_argument("--tune-cache", default=None, metavar="FILE", dest="tune_cache",
                    help="--cache: sweep --thetas x --lams on FILE (the dev set) and report the test perplexity at the best pair")
    ap.add_argument("--thetas", default=",".join("%.1f" % (0.1 * i) for i in range(11)), help="--tune-cache: the thetas of the grid")
    ap.add_argument("--lams", default=",".join("%.2f" % (0.05 * i) for i in range(20)), help="--tune-cache: the lams of the grid")
    ap.add_argument("--dynamic", action="store_true",
                    help="stream mode: also report the dynamically evaluated perplexity -- one gradient step per chunk (jlm_amd/dyneval.py)")
    ap.add_argument("--de-rule", choices=("sgd", "rms"), default="sgd", dest="de_rule", help="--dynamic: the update rule")
    ap.add_argument("--de-lr", type=float, default=0.005, dest="de_lr", help="--dynamic: the learning rate")
    ap.add_argument("--de-lam", type=float, default=0.02, dest="de_lam", help="--dynamic: the decay towards the loaded weights, in [0, 1)")
    ap.add_argument("--de-eps", type=float, default=1e-3, dest="de_eps", help="--dynamic, rule rms: what is added to RMS")
    ap.add_argument("--de-steps", type=int, default=5, dest="de_steps", help="--dynamic: tokens per chunk, i.e. per update")
    ap.add_argument("--de-stat-chunks", type=int, default=500, dest="de_stat_chunks",
                    help="--dynamic, rule rms: chunks of data/train.txt the gradient statistics are taken over")
    ap.add_argument("--tune-dynamic", default=None, metavar="FILE", dest="tune_dynamic",
                    help="--dynamic: sweep --de-lrs x --de-lams on FILE (the dev set) and report the test perplexity at the best pair")
    ap.add_argument("--de-lrs", default="0.001,0.002,0.005,0.01,0.02", dest="de_lrs", help="--tune-dynamic: the learning rates of the grid")
    ap.add_argument("--de-lams", default="0,0.01,0.02,0.05", dest="de_lams", help="--tune-dynamic: the decays of the grid")
    ap.add_argument("--ngram", default=None, metavar="FILE",
                    help="stream mode: also report the perplexity of the mixture with the back-off n-gram model of FILE (SRILM text, "
                         "python -m jlm_amd.ngram), formed on the host in float64 from score_streams' -log p: no new kernel runs")
    ap.add_argument("--ngram-order", type=int, default=3, dest="ngram_order", help="--ngram: the order FILE is read at")
    ap.add_argument("--ngram-lam", type=float, default=0.3, dest="ngram_lam", help="--ngram: the n-gram model's weight")
    ap.add_argument("--tune-ngram", default=None, metavar="DEV", dest="tune_ngram", help="--ngram: pick lambda on this text file over --ngram-lams")
    ap.add_argument("--ngram-lams", default=",".join("%.2f" % (0.05 * i) for i in range(1, 20)), dest="ngram_lams",
                    help="--tune-ngram: the lambdas of the grid")
    ap.add_argument("--memory", default=None, metavar="MEM", help="stream mode: also report the perplexity under the memory saved in MEM")
    ap.add_argument("--mem-theta", type=float, default=0.3, dest="mem_theta", help="--memory: the flatness of the memory's distribution")
    ap.add_argument("--mem-lam", type=float, default=0.1, dest="mem_lam", help="--memory: the weight of the memory in the mixture")
    ap.add_argument("--tune-memory", default=None, metavar="DEV", dest="tune_memory",
                    help="--memory: sweep --thetas x --lams on DEV (the dev set) and report the test perplexity at the best pair")
    ap.add_argument("--mem-k", type=int, default=None, dest="mem_k", metavar="K",
                    help="--memory with --ranks: a second --ranks line under the memory's K nearest entries (1 .. 1024)")
    args = ap.parse_args(argv)
    if args.mem_k is not None and not (args.memory and args.ranks and 1 <= args.mem_k <= 1024):
        ap.error("--mem-k K (1 .. 1024) goes with --memory and --ranks")
    if args.tune_memory and not args.memory:
        ap.error("--tune-memory goes with --memory")
    mem_spec = mem_tune_spec = None
    if args.memory:
        from .cache import check_lam as _check_lam
        from .memory import MemorySpec
        if args.mode != "stream" or args.cache or args.tune_cache or args.dynamic or args.ngram:
            ap.error("--memory works in stream mode, without --cache, --dynamic and --ngram")
        try:
            mem_spec = MemorySpec(args.mem_theta, args.mem_lam)
            if args.tune_memory:
                mem_tune_lams = [_check_lam(x) for x in _floats(args.lams, "--lams", ap)]
                if not mem_tune_lams:
                    ap.error("--lams is empty")
                mem_tune_spec = MemorySpec(_floats(args.thetas, "--thetas", ap))
        except ValueError as e:
            ap.error(str(e))
    if args.tune_ngram and not args.ngram:
        ap.error("--tune-ngram goes with --ngram")
    ngram_lams = None
    if args.ngram:
        if args.mode != "stream" or args.dynamic:
            ap.error("--ngram works in stream mode, without --dynamic")
        ngram_lams = _floats(args.ngram_lams, "--ngram-lams", ap) if args.tune_ngram else [args.ngram_lam]
        if not ngram_lams or not all(0.0 < x < 1.0 for x in ngram_lams) or args.ngram_order not in (1, 2, 3):
            ap.error("--ngram-lam / --ngram-lams lie in (0, 1), --ngram-order is 1, 2 or 3")
    if args.tune_dynamic and not args.dynamic:
        ap.error("--tune-dynamic goes with --dynamic")
    de_spec = de_grid = None
    if args.dynamic:
        from . import dyneval as _de
        if args.mode != "stream" or args.cache or args.tune_cache or args.ranks:
            ap.error("--dynamic works in stream mode, without --cache and --ranks")
        if args.comp:
            ap.error("--dynamic runs on the uncompressed weights")
        try:
            de_spec = _de.DynEvalSpec(args.de_lr, args.de_lam, args.de_rule, args.de_eps, args.batch_size or 1, args.de_steps)
            _de.check_spec(de_spec, stats={} if args.de_rule == "rms" else None)
            if args.de_rule == "rms" and args.de_stat_chunks < 1:
                ap.error("--de-stat-chunks takes an integer >= 1")
            if args.tune_dynamic:
                de_grid = (_floats(args.de_lrs, "--de-lrs", ap), _floats(args.de_lams, "--de-lams", ap))
                if not de_grid[0] or not de_grid[1]:
                    ap.error("--de-lrs or --de-lams is empty")
                for lr in de_grid[0]:
                    for lam in de_grid[1]:
                        _de.check_spec(de_spec.replace(lr=lr, lam=lam), stats={} if args.de_rule == "rms" else None)
        except ValueError as e:
            ap.error(str(e))
    spec = tune_spec = None
    if args.cache or args.tune_cache:
        from .cache import CacheSpec, check_lam
        if args.mode != "stream" or args.cache < 1:
            ap.error("--cache N (N >= 1) and --tune-cache work in stream mode")
        try:
            spec = CacheSpec(args.cache, args.theta, args.lam)
            if args.tune_cache:
                tune_lams = [check_lam(x) for x in _floats(args.lams, "--lams", ap)]
                if not tune_lams:
                    ap.error("--lams is empty")
                tune_spec = CacheSpec(args.cache, _floats(args.thetas, "--thetas", ap))
        except ValueError as e:
            ap.error(str(e))
    tops = [int(k) for k in args.top.split(",") if k.strip()]
    if args.ranks and (not tops or min(tops) < 1 or args.list_size < 1):
        ap.error("--top and --list take integers >= 1")
    if args.ranks and spec is not None and spec.size > 4096:
        ap.error("--ranks with --cache takes a cache of at most 4096 entries")
    config, vocab = load_vocab(args)
    from .model import LSTM_Model
    path = args.file or os.path.join(_config.data_path, "test.txt")
    sents, n_unk = encode_lines(read_lines(path, args.es), vocab)
    model = None if de_stepper == "reference" else LSTM_Model(experiment_id=args.experiment_id, comp=args.comp)
    t0 = time.time()
    if args.mode == "sentence":
        pp, _total, n_tok = sentence_perplexity(model, sents, vocab.t2i["<eos>"])
    else:
        bs = args.batch_size or (1 if args.dynamic else int(config.get("batch_size", 64)))
        stream = [i for s in sents for i in s]
        if model is None:
            pp, _total, n_tok = _de.dynamic_perplexity(args.experiment_id, stream, _de.DynEvalSpec(0.0, batch_size=bs, num_steps=args.num_steps),
                                                       stepper=de_stepper)
        elif mem_spec is not None:
            from .memory import Memory, MemorySpec, tune as mem_tune
            try:
                memory = Memory.load(model, args.memory)
            except (ValueError, OSError) as e:
                ap.error(str(e))
            if mem_tune_spec is not None:
                dev_sents, _n = encode_lines(read_lines(args.tune_memory), vocab)
                dev_parts = stream_memory_scores(model, [i for s in dev_sents for i in s], bs, args.num_steps, memory, mem_tune_spec)
                best_theta, best_lam = mem_tune(dev_parts, mem_tune_lams)
                mem_dev_pp = cached_perplexity(dev_parts, best_lam, mem_tune_spec.thetas.index(best_theta))
                mem_spec = MemorySpec(best_theta, best_lam)
                t0 = time.time()
            pp, mem_pp, n_tok = cached_perplexity(stream_memory_scores(model, stream, bs, args.num_steps, memory, mem_spec), mem_spec.lam)
        elif spec is None:
            pp, _total, n_tok = stream_perplexity(model, stream, bs, args.num_steps)
        else:
            if tune_spec is not None:
                from .cache import tune
                dev_sents, _n = encode_lines(read_lines(args.tune_cache), vocab)
                dev_parts = stream_cached_scores(model, [i for s in dev_sents for i in s], bs, args.num_steps, tune_spec)
                best_theta, best_lam = tune(dev_parts, tune_lams)
                dev_pp = cached_perplexity(dev_parts, best_lam, tune_spec.thetas.index(best_theta))
                spec = CacheSpec(args.cache, best_theta, best_lam)
                t0 = time.time()
            pp, cached_pp, n_tok = cached_perplexity(stream_cached_scores(model, stream, bs, args.num_steps, spec), spec.lam)
    dt = time.time() - t0
    print("tokens: {}  <unk>: {}  tokens/s: {:.0f}".format(n_tok, n_unk, n_tok / dt if dt > 0 else float("inf")))
    print("Test perplexity: {}".format(pp))
    if tune_spec is not None:
        print("Cache tuned on {}: theta {} lam {}  (dev perplexity {} -> {} over {} x {} pairs)".format(
            args.tune_cache, spec.theta, spec.lam, dev_pp[0], dev_pp[1], len(tune_spec.thetas), len(tune_lams)))
    if spec is not None:
        print("Test perplexity with cache (N {} theta {} lam {}): {}".format(spec.size, spec.theta, spec.lam, cached_pp))
    if mem_tune_spec is not None:
        print("Memory tuned on {}: theta {} lam {}  (dev perplexity {} -> {} over {} x {} pairs)".format(
            args.tune_memory, mem_spec.theta, mem_spec.lam, mem_dev_pp[0], mem_dev_pp[1], len(mem_tune_spec.thetas), len(mem_tune_lams)))
    if mem_spec is not None:
        print("Test perplexity with memory (N {} theta {} lam {}): {}".format(memory.N, mem_spec.theta, mem_spec.lam, mem_pp))
    if args.ngram:
        from .ngram import NGramTable
        ng_path = args.ngram if os.path.exists(args.ngram) else os.path.join(_config.data_path, args.ngram)
        table = NGramTable.from_srilm(ng_path, vocab.t2i, args.ngram_order)
        ng_lam = args.ngram_lam
        if args.tune_ngram:
            dev_sents, _n = encode_lines(read_lines(args.tune_ngram), vocab)
            dev_nll, dev_q = stream_ngram_scores(model, [i for s in dev_sents for i in s], bs, args.num_steps, table)
            grid = [ngram_mixture_perplexity(dev_nll, dev_q, x) for x in ngram_lams]
            ng_lam = ngram_lams[int(np.argmin(grid))]
            print("N-gram mixture tuned on {}: lam {}  (dev perplexity {} -> {} over {} values)".format(
                args.tune_ngram, ng_lam, float(np.exp(dev_nll.mean())), min(grid), len(grid)))
        ng_nll, ng_q = stream_ngram_scores(model, stream, bs, args.num_steps, table)
        print("Test perplexity with n-gram mixture (order {} lam {}; host float64 over score_streams' -log p): {}".format(
            table.order, ng_lam, ngram_mixture_perplexity(ng_nll, ng_q, ng_lam)))
    if de_spec is not None:
        stats = None
        if de_spec.rule == "rms":
            train_sents, _n = encode_lines(read_lines(os.path.join(_config.data_path, "train.txt")), vocab)
            stats = _de.experiment_stats(args.experiment_id, [i for s in train_sents for i in s], args.de_stat_chunks, bs, args.de_steps,
                                         stepper=de_stepper)
        if de_grid is not None:
            dev_sents, _n = encode_lines(read_lines(args.tune_dynamic), vocab)
            grid, (best_lr, best_lam) = _de.tune(args.experiment_id, [i for s in dev_sents for i in s], de_grid[0], de_grid[1], de_spec.rule,
                                                 de_spec.eps, bs, args.de_steps, stats=stats, stepper=de_stepper)
            de_spec = de_spec.replace(lr=best_lr, lam=best_lam)
            print("Dynamic evaluation tuned on {}: lr {} lam {}  (dev perplexity {} over {} x {} pairs)".format(
                args.tune_dynamic, best_lr, best_lam, float(grid.min()), grid.shape[0], grid.shape[1]))
        t0 = time.time()
        de_pp, _total, de_tok = _de.dynamic_perplexity(args.experiment_id, stream, de_spec, stats=stats, stepper=de_stepper)
        dt = time.time() - t0
        print("Test perplexity with dynamic evaluation (rule {} lr {} lam {} chunks of {} x {}; {} tokens, {:.0f} tokens/s): {}".format(
            de_spec.rule, de_spec.lr, de_spec.lam, bs, args.de_steps, de_tok, de_tok / dt if dt > 0 else float("inf"), de_pp))
    if args.ranks:
        readings = not isinstance(vocab, CharVocab)
        if args.mode == "sentence":
            ranks, targets = sentence_ranks(model, sents, vocab.t2i["<eos>"], readings, args.max_prefix)
        else:
            ranks, targets = stream_ranks(model, stream, bs, args.num_steps, readings, args.max_prefix)
        print(ranks_line(ranks, targets, model.reading_index() if readings else None, tops, args.list_size))
        if spec is not None:
            ranks, targets = stream_ranks(model, stream, bs, args.num_steps, readings, args.max_prefix, spec)
            print("with cache (N {} theta {} lam {}): ".format(spec.size, spec.theta, spec.lam) +
                  ranks_line(ranks, targets, model.reading_index() if readings else None, tops, args.list_size))
        if args.ngram:
            from .ngram import NGramMix
            ranks, targets = stream_ranks(model, stream, bs, args.num_steps, readings, args.max_prefix, ngram=NGramMix(table, ng_lam))
            print("with n-gram (order {} lam {}): ".format(table.order, ng_lam) +
                  ranks_line(ranks, targets, model.reading_index() if readings else None, tops, args.list_size))
        if args.mem_k is not None:
            from .memory import MemoryMix
            mix = MemoryMix(memory, mem_spec.theta, mem_spec.lam, args.mem_k)
            ranks, targets = stream_ranks(model, stream, bs, args.num_steps, readings, args.max_prefix, memory=mix)
            print("with memory (N {} K {} theta {} lam {}): ".format(memory.N, mix.k, mix.theta, mix.lam) +
                  ranks_line(ranks, targets, model.reading_index() if readings else None, tops, args.list_size))
    return pp


if __name__ == "__main__":
    main()
