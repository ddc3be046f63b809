"""Throughput of beam-search completion on the device (LSTM_Model.complete, csrc jlm_complete_frames): one JSON line.

  models          mid-vtable (BASELINE configs[1]'s model, V = 50 000) and mid-tied (tied softmax, V = 50 000)
  rows            256, 1 024 and 2 560 rows (prompts x beam, beam 8 by default) from <eos>, 10 words each
  per frame       event-time medians over the selecting frames after the first (Completer.run(timed=True)): LSTM step, T projection,
                  logit GEMMs, row selection (topk_rows_kernel), merge (beam_merge_kernel), and each one's share of the frame;
                  words/s from the events (rows expanded per second of frame)
  baseline        the host form of one next-word query: predict() and an argsort of the [1, V] distribution (the reference's
                  find_top_N) at one row

  --reading       instead: prediction from a typed reading prefix on mid-vtable.  256, 1 024 and 2 560 contexts from <eos>, context p
                  restricted to the words whose reading starts with kana p % 80 (LSTM_Model.predict_reading): the event time of the
                  first frame's selection with the sets (topk_rows_masked_kernel) beside the same rows' unrestricted selection
                  (topk_rows_kernel), alternating, median and range of the repeats; queries/s of predict_reading; and the host form of
                  one such query: predict(), a Python filter to the set and an argsort, at one row

    python tools/complete_bench.py [--root DIR] [--repeats N] [--beam B] [--words N] [--quick] [--reading]

words/s = rows x words / wall seconds of the call (upload, launches, read-back of the back-pointers, backtrace), median of the
repeats after one warm-up call.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def _model(root, name):
    from jlm_amd import config as jconfig, synth
    d = os.path.join(root, name)
    if not os.path.exists(os.path.join(d, "train", "experiments", "1", "config.json")):
        synth.build_fixture(d, name)
    jconfig.set_root(d)
    from jlm_amd.model import LSTM_Model
    return d, LSTM_Model(experiment_id=1)


def _median_time(fn, repeats):
    fn()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def reading_leg(root, reps, B, quick):
    """the --reading leg: see the module docstring"""
    import torch
    from jlm_amd import complete as C, synth
    _d, model = _model(root, "mid-vtable")
    m = model.dev
    index = model.reading_index()
    comp = C.Completer(m)
    res = {"V": m.V, "beam": B}
    stat = lambda a: {"median_us": round(float(np.median(a)) * 1e3, 2), "min_us": round(float(np.min(a)) * 1e3, 2),
                      "max_us": round(float(np.max(a)) * 1e3, 2)}
    for R in (256, 1024, 2560):
        ctx = [np.array([C.EOS_ID])] * R
        prefixes = [synth.KANA[p % len(synth.KANA)] for p in range(R)]
        sets = [index.lookup(x) for x in prefixes]

        def select_ms(first_sets):
            comp.run(ctx, 1, B, timed=True, first_sets=first_sets)
            return comp.last_frame_ms[0][3]              # frame 0's selection bracket

        select_ms(None), select_ms(sets)
        plain, masked = [], []
        for _ in range(reps):                            # alternating: the two see the same machine
            plain.append(select_ms(None))
            masked.append(select_ms(sets))
        t = _median_time(lambda: model.predict_reading([[C.EOS_ID]] * R, prefixes, n=B), reps)
        res["rows_%d" % R] = {"set_words_mean": round(float(np.mean([len(s) for s in sets])), 1), "select_unmasked": stat(plain),
                              "select_masked": stat(masked),
                              "masked_over_unmasked": round(float(np.median(masked) / np.median(plain)), 4),
                              "predict_reading_s": round(t, 5), "queries_per_s": round(R / t, 1)}
        torch.cuda.empty_cache()
    n_host = 10 if quick else 50
    allowed = index.lookup(synth.KANA[0])
    model.hidden = np.zeros((1, m.H))
    model.cell = np.zeros((1, m.H))
    model.predict([C.EOS_ID])
    t0 = time.perf_counter()
    for _ in range(n_host):
        pred = model.predict([C.EOS_ID])[0]
        allowed[np.argsort(-pred[0][allowed])[:B]]       # the filter and argsort a caller without the device path writes
    t = time.perf_counter() - t0
    res["host_predict_filter_argsort_1_row"] = {"queries": n_host, "s": round(t, 4), "queries_per_s": round(n_host / t, 1)}
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", default=None, help="fixture directory (default: a temporary one)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--beam", type=int, default=8)
    ap.add_argument("--words", type=int, default=10)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--reading", action="store_true", help="the reading-prefix leg instead of the completion one")
    args = ap.parse_args(argv)
    root = args.root or tempfile.mkdtemp(prefix="jlm_complete_bench_")
    reps = 2 if args.quick else args.repeats
    N, B = args.words, args.beam
    import torch
    from jlm_amd import complete as C
    if args.reading:
        out = {"bench": "complete-reading", "device": torch.cuda.get_device_name(0), "mid-vtable": reading_leg(root, reps, B, args.quick)}
        print(json.dumps(out))
        return out
    out = {"bench": "complete", "device": torch.cuda.get_device_name(0), "words_per_row": N, "beam": B}
    parts = ("lstm", "t_proj", "logit_gemm", "select", "merge")
    for name in ("mid-vtable", "mid-tied"):
        _d, model = _model(root, name)
        m = model.dev
        res = out[name] = {"V": m.V}
        comp = C.Completer(m)
        for R in (256, 1024, 2560):
            n_prompts = max(1, R // B)
            prompts = [[C.EOS_ID]] * n_prompts
            t = _median_time(lambda: model.complete(prompts, N, beam_width=B), reps)
            comp.run([np.array([C.EOS_ID])] * n_prompts, N, B, timed=True)
            ms = comp.last_frame_ms[1:]                 # [frames, 5]; frame 0 selects from the prompts' rows alone
            med = np.median(ms, axis=0)
            tot = float(med.sum())
            rows = n_prompts * B
            res["rows_%d" % rows] = {"prompts": n_prompts, "words": rows * N, "s": round(t, 5), "words_per_s": round(rows * N / t, 1),
                                     "frame_us": dict({p: round(float(v) * 1e3, 2) for p, v in zip(parts, med)}, total=round(tot * 1e3, 2)),
                                     "frac": {p: round(float(v) / tot, 4) for p, v in zip(parts, med)},
                                     "words_per_s_from_events": round(rows / (tot * 1e-3), 1)}
        if name == "mid-vtable":
            n_host = 10 if args.quick else 50
            model.hidden = np.zeros((1, m.H))
            model.cell = np.zeros((1, m.H))
            model.predict([C.EOS_ID])
            t0 = time.perf_counter()
            for _ in range(n_host):
                pred = model.predict([C.EOS_ID])[0]
                np.argsort(-pred[0])[:B]
            t = time.perf_counter() - t0
            res["host_predict_argsort_1_row"] = {"queries": n_host, "s": round(t, 4), "queries_per_s": round(n_host / t, 1)}
            ctx = [[C.EOS_ID]] * 256
            t = _median_time(lambda: model.predict_top(ctx, n=B), reps)
            res["predict_top_256_contexts"] = {"s": round(t, 5), "queries_per_s": round(256 / t, 1)}
        del model, m, comp
        torch.cuda.empty_cache()
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
