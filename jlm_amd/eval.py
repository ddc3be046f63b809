"""Evaluation harness: counterpart of the reference's decoder/eval.py.

Same flags (eval.py:17-28, including the ``type=bool`` behaviour: any non-empty
string is true), same decoder selection order (eval.py:41-48), same eval-set
loader (eval.py:125-166), same log file name/body and the same printed summary
lines (eval.py:65-122) -- those strings are the file format the golden vectors
pin.  Extras: ``--root`` (artefact directory; the reference freezes it from
``__file__``), ``--batch N`` decodes N sentences per GPU launch sequence instead
of one (identical output, much faster), ``--context_words N`` (``-cw``) converts every
sentence in the middle of its text: its first min(N, words - 1) gold words are the
left context (``Decoder.decode(context=)``), the kana of the rest is the input and
the hit is judged on the rest's surface; the log name gains ``_ctx_N``.  With 0
(the default) name and body of the log are what they were.  ``--cut_last N`` drops
the last N kana of every sentence's reading -- the last word is unfinished, as
while the user types -- converts it with ``Decoder.decode_predict`` and judges the
PREDICTIONS: how often the full target string is the first prediction, among
them, or missed -- the keystrokes a model saves; the log name gains ``_cut_N``.

    python -m jlm_amd.eval --root /path/to/artifacts -e 1 -es 100 -b 10 [--batch 256]
"""
import argparse
import os
import time

import numpy as np

from . import config as _config
from .data import Vocab

# (long flag, short flag, type, default, what it selects) -- eval.py:17-28
_FLAGS = [
    ("experiment_id", "e", int, 1, "experiment directory under train/experiments/"),
    ("eval_size", "es", int, 100, "sentences taken from data/test.txt"),
    ("use_ngram", "ng", bool, False, "decode with the n-gram baseline instead of the LSTM"),
    ("ngram_order", "o", int, 3, "order of the n-gram model"),
    ("comp", "c", int, 0, "bits of the k-means compressed weights to load (0: uncompressed)"),
    ("vocab_select", "vs", bool, False, "normalise over the lattice's own words only"),
    ("top_sampling", "ts", bool, False, "add the `samples` most frequent words to the selected vocabulary"),
    ("random_sampling", "rs", bool, False, "add `samples` random words to the selected vocabulary"),
    ("samples", "s", int, 0, "number of sampled words"),
    ("beam_size", "b", int, 10, "hypotheses kept per frame"),
    ("dynamic_decoding", "dd", bool, False, "incremental vocabulary selection (DynamicDecoder)"),
]
_LOG_NAME = 'eval/eval_log_{}_e_{}_dynamic_{}_size_{}_b_{}_comp_{}_vocab_sel_{}_samples_{}_top_{}_random_{}.txt'


def build_parser():
    parser = argparse.ArgumentParser(description="conversion accuracy of a decoder on data/test.txt")
    for name, short, typ, default, text in _FLAGS:
        parser.add_argument("--" + name, "-" + short, type=typ, default=default, help=text)
    parser.add_argument("--root", default=None, help="artefact root (data/, train/experiments/)")
    parser.add_argument("--batch", type=int, default=1, help="sentences decoded per batch on the GPU")
    parser.add_argument("--context_words", "-cw", type=int, default=0,
                        help="gold words of every sentence given to the decoder as left context (the rest is converted)")
    parser.add_argument("--cache", type=int, default=0,
                        help="with --context_words: decode the set a second time under a continuous cache of N entries over every "
                             "sentence's context (Decoder.decode(cache=)) and log both summaries")
    parser.add_argument("--theta", type=float, default=0.3, help="--cache: the cache's theta")
    parser.add_argument("--lam", type=float, default=0.1, help="--cache: the cache's lambda")
    parser.add_argument("--ngram_mix", default=None,
                        help="decode the set a second time with the back-off n-gram model of this file (SRILM text, python -m "
                             "jlm_amd.ngram; read at --ngram_order) mixed into every edge cost (Decoder.decode(ngram=)) and log both summaries")
    parser.add_argument("--ngram_lam", type=float, default=0.3, help="--ngram_mix: the n-gram model's weight lambda")
    parser.add_argument("--cut_last", type=int, default=0,
                        help="drop the last N kana of every reading and count how often the full target is among the predictions of "
                             "the unfinished last word (Decoder.decode_predict)")
    # (no attribute without the flag: the namespace of a run that does not ask for it is what it was)
    parser.add_argument("--candidates", type=int, default=argparse.SUPPRESS,
                        help="for sentences whose best conversion has the gold segmentation but a wrong string: where the gold word "
                             "stands in each wrong segment's list of N candidates (Decoder.decode_candidates)")
    parser.add_argument("--memory", default=argparse.SUPPRESS,
                        help="decode the set a second time under the memory of hidden states saved in this .npz (python -m jlm_amd.memory; "
                             "Decoder.decode(memory=)) and log both summaries")
    parser.add_argument("--mem-theta", dest="mem_theta", type=float, default=argparse.SUPPRESS, help="--memory: theta (default 0.3)")
    parser.add_argument("--mem-lam", dest="mem_lam", type=float, default=argparse.SUPPRESS, help="--memory: the memory's weight lambda (default 0.1)")
    parser.add_argument("--mem-k", dest="mem_k", type=int, default=argparse.SUPPRESS, help="--memory: the nearest entries that vote (default 64)")
    return parser


def _surface(token):
    return token.split('/')[0]


def _reading(token):
    parts = token.split('/')
    return parts[1] if parts[1] != '' else parts[0]


class Evaluator:
    def __init__(self, args):
        self.args = args
        self.config = _config.load_config_dict(args.experiment_id)
        if self.config['char_rnn']:          # eval.py:35-36
            from .data import CharVocab
            self.vocab = CharVocab(self.config['vocab_size'])
        else:
            self.vocab = Vocab(self.config['vocab_size'])
        self.w2i = self.vocab.w2i
        self.context_words = max(0, int(getattr(args, "context_words", 0) or 0))
        if self.context_words and (args.use_ngram or self.config['char_rnn']):
            raise ValueError("--context_words: the n-gram and character decoders take no left context")
        self.cut_last = max(0, int(getattr(args, "cut_last", 0) or 0))
        if self.cut_last and (args.use_ngram or self.config['char_rnn'] or args.dynamic_decoding or args.vocab_select):
            raise ValueError("--cut_last: the last word is predicted by the static decoder over the full vocabulary")
        self.cache = None                # --cache N: the CacheSpec of the second pass
        if int(getattr(args, "cache", 0) or 0):
            if not self.context_words or args.dynamic_decoding or args.vocab_select or self.cut_last:
                raise ValueError("--cache needs --context_words and the static decoder over the full vocabulary")
            from .cache import CacheSpec
            from .context import check_decode_cache
            self.cache = check_decode_cache(CacheSpec(int(args.cache), theta=float(args.theta), lam=float(args.lam)))
        self.ngram_mix = None            # --ngram_mix FILE: the NGramMix of the second pass
        if getattr(args, "ngram_mix", None):
            if args.use_ngram or self.config['char_rnn'] or args.dynamic_decoding or args.vocab_select or self.cut_last or self.cache is not None:
                raise ValueError("--ngram_mix needs the static decoder over the full vocabulary, without --cache and --cut_last")
            from .ngram import NGramMix, NGramTable, check_mix
            path = args.ngram_mix if os.path.isabs(args.ngram_mix) or os.path.exists(args.ngram_mix) else os.path.join(_config.data_path, args.ngram_mix)
            self.ngram_mix = check_mix(NGramMix(NGramTable.from_srilm(path, self.w2i, int(args.ngram_order)), float(args.ngram_lam)), len(self.w2i))
        self.candidates = max(0, int(getattr(args, "candidates", 0) or 0))
        if self.candidates and (args.use_ngram or self.config['char_rnn'] or args.dynamic_decoding or args.vocab_select or self.cut_last or
                                self.cache is not None or self.ngram_mix is not None):
            raise ValueError("--candidates: the segments' lists come from the static decoder over the full vocabulary, without --cut_last, "
                             "--cache and --ngram_mix")
        if self.candidates > 64:
            raise ValueError("--candidates: at most 64 words per segment")
        self.memory_mix = None           # --memory MEM.npz: the MemoryMix of the second pass (loaded behind the decoder, below)
        if getattr(args, "memory", None) and (args.use_ngram or self.config['char_rnn'] or args.dynamic_decoding or args.vocab_select or
                                              self.cut_last or self.candidates or self.cache is not None or self.ngram_mix is not None):
            raise ValueError("--memory needs the static decoder over the full vocabulary, without --cache, --ngram_mix, --cut_last and "
                             "--candidates")
        self.contexts = None             # with --context_words: every loaded sentence's context tokens (load_eval_set)
        self.gold = None                 # with --candidates: every loaded sentence's gold tokens (load_eval_set)
        self.decoder = self._make_decoder()
        if hasattr(self.decoder, "perf_timing"):
            self.decoder.perf_timing = True       # the log's per-step times (eval.py:104-121) need the per-frame events
        if getattr(args, "memory", None):
            from .memory import Memory, MemoryMix
            self.memory_mix = MemoryMix(Memory.load(self.decoder.model, args.memory), theta=float(getattr(args, "mem_theta", 0.3)),
                                        lam=float(getattr(args, "mem_lam", 0.1)), k=int(getattr(args, "mem_k", 64)))

    def _make_decoder(self):
        a = self.args                 # selection order of eval.py:41-48
        if a.use_ngram:
            from .decoder_ngram import NGramDecoder
            return NGramDecoder(experiment_id=a.experiment_id, ngram_order=a.ngram_order)
        if self.config['char_rnn']:
            from .decoder_char import CharRNNDecoder
            return CharRNNDecoder(experiment_id=a.experiment_id, comp=a.comp)
        if a.dynamic_decoding:
            from .decoder_dynamic import DynamicDecoder
            return DynamicDecoder(experiment_id=a.experiment_id, comp=a.comp)
        from .decoder import Decoder
        return Decoder(experiment_id=a.experiment_id, comp=a.comp)

    def log_name(self):
        a = self.args
        kind = "ngram_{}".format(a.ngram_order) if a.use_ngram else "neural"
        name = _LOG_NAME.format(kind, a.experiment_id, a.dynamic_decoding, a.eval_size, a.beam_size, a.comp, a.vocab_select,
                                a.samples, a.top_sampling, a.random_sampling)
        if self.context_words:
            name = name[:-len(".txt")] + "_ctx_{}.txt".format(self.context_words)
        if self.cut_last:
            name = name[:-len(".txt")] + "_cut_{}.txt".format(self.cut_last)
        if self.cache is not None:
            name = name[:-len(".txt")] + "_cache_{}.txt".format(self.cache.size)
        if getattr(self, "ngram_mix", None) is not None:
            name = name[:-len(".txt")] + "_ngmix_{}.txt".format(self.ngram_mix.table.order)
        if getattr(self, "candidates", 0):
            name = name[:-len(".txt")] + "_cand_{}.txt".format(self.candidates)
        if getattr(self, "memory_mix", None) is not None:
            name = name[:-len(".txt")] + "_memory.txt"
        return name

    def _decode_all(self, inputs, cache=None, ngram=None, memory=None):
        a = self.args
        kw = dict(beam_width=a.beam_size, vocab_select=a.vocab_select, samples=a.samples,
                  top_sampling=a.top_sampling, random_sampling=a.random_sampling)
        if cache is not None:
            kw["cache"] = cache
        if ngram is not None:
            kw["ngram"] = ngram
        if memory is not None:
            kw["memory"] = memory
        step = max(1, a.batch)
        ctx = self.contexts if self.context_words else None
        if step == 1:                 # sentence at a time, as the reference does
            if ctx is not None:
                return [self.decoder.decode(x, context=c, **kw) for x, c in zip(inputs, ctx)]
            return [self.decoder.decode(x, **kw) for x in inputs]
        out = []
        for i in range(0, len(inputs), step):
            if ctx is not None:
                out.extend(self.decoder.decode_batch(inputs[i:i + step], context=ctx[i:i + step], **kw))
            else:
                out.extend(self.decoder.decode_batch(inputs[i:i + step], **kw))
        return out

    def _predict_all(self, inputs):
        """the predictions of every input's unfinished last word (--cut_last)"""
        a = self.args
        step = max(1, a.batch)
        ctx = self.contexts if self.context_words else None
        out = []
        for i in range(0, len(inputs), step):
            res = self.decoder.decode_predict_batch(inputs[i:i + step], beam_width=a.beam_size,
                                                    context=ctx[i:i + step] if ctx is not None else None)
            out.extend(pred for _conv, pred in res)
        return out

    def evaluate_cut(self):
        """--cut_last N: -> (first prediction hits, hits further down the list, misses); the three add up to the sentences loaded"""
        n = self.cut_last
        hits = {"best hit": 0, "nbest hit": 0, "no hit": 0}
        with open(self.log_name(), 'w', encoding='utf-8') as log:
            inputs, targets = self.load_eval_set()
            cut = [x[:max(len(x) - n, 0)] for x in inputs]
            t_start = time.time()
            for x, y, preds in zip(cut, targets, self._predict_all(cut)):
                sentences = [''.join(_surface(w) for w in words) for _score, words in preds]
                verdict = "best hit" if sentences and y == sentences[0] else ("nbest hit" if y in sentences else "no hit")
                hits[verdict] += 1
                log.write(verdict + '\n')
                log.write('{}\t{}\n'.format(y, x))
                log.writelines(s + '\n' for s in sentences)
            summary = 'cut_last {} pred_best_hit {} pred_nbest_hit {} pred_miss {} eval_size {}'.format(
                n, hits["best hit"], hits["nbest hit"], hits["no hit"], len(inputs))
            log.write(summary)
            log.write("--- %s seconds ---" % (time.time() - t_start))
            print(summary)
            print("--- %s seconds ---" % (time.time() - t_start))
        return hits["best hit"], hits["nbest hit"], hits["no hit"]

    def evaluate_candidates(self):
        """--candidates N: the sentences whose 1-best has the gold segmentation but another string; for every wrong segment the position
        of the gold word in the segment's list.  -> (such sentences, wrong segments, those with the gold word at position <= 1, <= 5,
        <= N, sentences every wrong segment's top N can fix)"""
        n, a = self.candidates, self.args
        step = max(1, a.batch)
        with open(self.log_name(), 'w', encoding='utf-8') as log:
            inputs, targets = self.load_eval_set()
            ctx = self.contexts if self.context_words else None
            t_start = time.time()
            res = []
            for i in range(0, len(inputs), step):
                res.extend(self.decoder.decode_candidates_batch(inputs[i:i + step], topN=1, beam_width=a.beam_size, n_cand=n,
                                                                context=ctx[i:i + step] if ctx is not None else None))
            sents = wrong = le1 = le5 = len_ = fixable = 0
            for x, y, gold, (conv, segs) in zip(inputs, targets, self.gold, res):
                best = conv[0][1] if conv else []
                spans, start = [], 0
                for t in gold:
                    spans.append((start, len(_reading(t))))
                    start += len(_reading(t))
                if ''.join(_surface(w) for w in best) == y or [(s, l) for s, l, _c in segs] != spans:
                    continue
                sents += 1
                log.write('{}\t{}\n'.format(y, x))
                ok = True
                for t, w, (s, l, cands) in zip(gold, best, segs):
                    if _surface(w) == _surface(t):
                        continue
                    wrong += 1
                    pos = next((k + 1 for k, (_sc, c) in enumerate(cands) if _surface(c) == _surface(t)), None)
                    le1 += pos is not None and pos <= 1
                    le5 += pos is not None and pos <= 5
                    len_ += pos is not None
                    ok = ok and pos is not None
                    log.write('{}+{} {} -> {} position {}\n'.format(s, l, _surface(w), _surface(t), pos if pos is not None else '-'))
                fixable += ok
            share = lambda k, of: (float(k) / of) if of else 0.0
            summary = ('candidates {} same_seg_wrong {} wrong_segments {} pos_le_1 {:.3f} pos_le_5 {:.3f} pos_le_{} {:.3f} fixable {:.3f} '
                       'eval_size {}').format(n, sents, wrong, share(le1, wrong), share(le5, wrong), n, share(len_, wrong),
                                              share(fixable, sents), len(inputs))
            log.write(summary)
            log.write("--- %s seconds ---" % (time.time() - t_start))
            print(summary)
            print("--- %s seconds ---" % (time.time() - t_start))
        return sents, wrong, le1, le5, len_, fixable

    def _timing_lines(self):
        a, d = self.args, self.decoder
        if a.use_ngram:               # eval.py:104-107: only the neural decoders log per-step times
            return []
        per_step = d.perf_log_lstm + d.perf_log_softmax
        return ["--- %f seconds lstm per step ---" % (np.mean(d.perf_log_lstm)),
                "--- %f seconds softmax per step ---" % (np.mean(d.perf_log_softmax)),
                "--- %f seconds per sent.---" % (np.sum(per_step) / d.perf_sen)]

    def evaluate(self):
        a = self.args
        hits = {"best hit": 0, "nbest hit": 0, "no hit": 0}
        with open(self.log_name(), 'w', encoding='utf-8') as log:
            inputs, targets = self.load_eval_set()
            t_start = time.time()
            for x, y, nbest in zip(inputs, targets, self._decode_all(inputs)):
                sentences = [''.join(_surface(w) for w in words) for _score, words in nbest]
                verdict = "best hit" if y == sentences[0] else ("nbest hit" if y in sentences else "no hit")
                hits[verdict] += 1
                log.write(verdict + '\n')
                log.write('{}\t{}\n'.format(y, x))
                log.writelines(s + '\n' for s in sentences)
            best, nbest_hits = hits["best hit"], hits["nbest hit"]
            summary = 'best_hit {} nbest_hit{} no_hit {} eval_size {}'.format(best, nbest_hits, a.eval_size - best - nbest_hits,
                                                                             a.eval_size)
            timing = self._timing_lines()
            log.write(summary)
            log.writelines(timing)
            log.write("--- %s seconds ---" % (time.time() - t_start))
            print(summary)
            for ln in timing:
                print(ln)
            if a.dynamic_decoding and not a.use_ngram:
                d = self.decoder
                fix = lambda v: ("%f" % np.mean(v)) if len(v) else "n/a"
                print("--- %s seconds per step for vocab fix.---" % fix(d.perf_log_fix_vocab))
                print("--- %s seconds per step for lattice path fix.---" % fix(d.perf_log_fix_lattice_path_prob))
            print("--- %s seconds ---" % (time.time() - t_start))
            mix, mem = getattr(self, "ngram_mix", None), getattr(self, "memory_mix", None)
            if self.cache is not None or mix is not None or mem is not None:
                # the same set once more under the cache (or the n-gram mixture, or the memory): its verdicts and its summary line behind
                # the first pass's
                hits = {"best hit": 0, "nbest hit": 0, "no hit": 0}
                t_start = time.time()
                log.write('\n')
                for x, y, nb in zip(inputs, targets, self._decode_all(inputs, cache=self.cache, ngram=mix, memory=mem)):
                    sentences = [''.join(_surface(w) for w in words) for _score, words in nb]
                    verdict = "best hit" if y == sentences[0] else ("nbest hit" if y in sentences else "no hit")
                    hits[verdict] += 1
                    log.write(verdict + '\n')
                    log.write('{}\t{}\n'.format(y, x))
                    log.writelines(s + '\n' for s in sentences)
                head = ('cache {} theta {} lam {}'.format(self.cache.size, self.cache.theta, self.cache.lam) if self.cache is not None
                        else 'ngram_mix order {} lam {}'.format(mix.table.order, mix.lam) if mix is not None
                        else 'memory {} theta {} lam {} k {}'.format(mem.memory.N, mem.theta, mem.lam, mem.k))
                summary = '{} best_hit {} nbest_hit{} no_hit {} eval_size {}'.format(
                    head, hits["best hit"], hits["nbest hit"], a.eval_size - hits["best hit"] - hits["nbest hit"], a.eval_size)
                log.write(summary)
                log.write("--- %s seconds ---" % (time.time() - t_start))
                print(summary)
                print("--- %s seconds ---" % (time.time() - t_start))
        return best, nbest_hits

    def load_eval_set(self):
        """The first ``eval_size`` lines of data/test.txt whose tokens are all in-vocabulary (eval.py:125-166):
        x = the tokens' readings (the surface where a token has none), y = their surfaces, both concatenated.  With
        --context_words N the first min(N, tokens - 1) tokens of a line go to ``self.contexts`` and x, y are those of the rest."""
        from .context import split_sentence
        want = self.args.eval_size
        xs, ys = [], []
        self.contexts = [] if self.context_words else None
        self.gold = [] if getattr(self, "candidates", 0) else None
        with open(os.path.join(_config.data_path, 'test.txt'), 'r', encoding='utf-8') as f:
            lines = f.readlines()
        print('take {} for evaluation from all {} lines'.format(want, len(lines)))
        for line in lines:
            tokens = line.strip().split(' ')
            if any(self.decoder._check_oov(t) for t in tokens):
                continue
            if self.context_words:
                ctx, tokens = split_sentence(tokens, self.context_words)
                self.contexts.append(ctx)
            if self.gold is not None:
                self.gold.append(list(tokens))
            xs.append(''.join(_reading(t) for t in tokens))
            ys.append(''.join(_surface(t) for t in tokens))
            if len(xs) >= want:
                break
        print('{} pairs load'.format(len(xs)))
        return xs, ys


def parse_log(top='./'):
    """Print the summary line of every eval log under ``top`` (eval.py:168-178)."""
    for folder, _subs, files in os.walk(top):
        for filename in files:
            if 'eval_log' not in filename:
                continue
            print(filename)
            with open(os.path.join(folder, filename), 'r', encoding='utf-8') as f:
                for line in f:
                    if 'best_hit' in line:
                        print(line.strip())


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.root:
        _config.set_root(args.root)
    os.makedirs('eval', exist_ok=True)
    ev = Evaluator(args)
    if ev.candidates:
        return ev.evaluate_candidates()
    return ev.evaluate_cut() if ev.cut_last else ev.evaluate()


if __name__ == '__main__':
    main()
