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


def main(argv=None):
    ap = argparse.ArgumentParser(description="Test perplexity of a dumped model on the device (reference train/train.py:101-102)")
    _config.add_model_args(ap)
    ap.add_argument("--file", default=None, help="text to score, one sentence per line (default: <root>/data/test.txt)")
    ap.add_argument("--mode", choices=("sentence", "stream"), default="stream")
    ap.add_argument("-b", "--batch_size", type=int, default=None, help="stream mode: parallel streams (default: the config's, else 64)")
    ap.add_argument("--num_steps", type=int, default=20, help="stream mode: steps per chunk")
    ap.add_argument("-es", type=int, default=0, help="score the first N lines only (0 = all)")
    args = ap.parse_args(argv)
    config, vocab = load_vocab(args)
    from .model import LSTM_Model
    path = args.file or os.path.join(_config.data_path, "test.txt")
    sents, n_unk = encode_lines(read_lines(path, args.es), vocab)
    model = LSTM_Model(experiment_id=args.experiment_id, comp=args.comp)
    t0 = time.time()
    if args.mode == "sentence":
        pp, _total, n_tok = sentence_perplexity(model, sents, vocab.t2i["<eos>"])
    else:
        bs = args.batch_size or int(config.get("batch_size", 64))
        stream = [i for s in sents for i in s]
        pp, _total, n_tok = stream_perplexity(model, stream, bs, args.num_steps)
    dt = time.time() - t0
    print("tokens: {}  <unk>: {}  tokens/s: {:.0f}".format(n_tok, n_unk, n_tok / dt if dt > 0 else float("inf")))
    print("Test perplexity: {}".format(pp))
    return pp


if __name__ == "__main__":
    main()
