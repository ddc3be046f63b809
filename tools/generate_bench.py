"""Throughput of batched sampling on the device (LSTM_Model.generate, csrc jlm_generate_frames): one JSON line.

  models          mid-vtable (BASELINE configs[1]'s model, V = 50 000) and mid-tied (tied softmax, V = 50 000)
  rows            256, 1 024 and 2 560 rows from <eos>, 20 draws each, temperature 1
  per frame       event times of LSTM step / T projection / logit GEMMs / draw at each row count (Generator.run(timed=True)),
                  the logit GEMMs' share of a frame, and tokens/s from the events
  truncation      the draw bracket and the frame with top_k = 40, top_p = 0.9 and both, beside the untruncated draw (the same
                  timed call; mid-vtable at 256 and 2 560 rows, mid-tied at 2 560)
  baseline        the host loop of model.main (one predict() and one sample() per word) at one row

    python tools/generate_bench.py [--root DIR] [--repeats N] [--quick]

tokens/s = drawn words / wall seconds of the call (upload, launches, read-back), median of the repeats after one warm-up call.
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


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", default=None, help="fixture directory (default: a temporary one)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--words", type=int, default=20)
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args(argv)
    root = args.root or tempfile.mkdtemp(prefix="jlm_generate_bench_")
    reps = 2 if args.quick else args.repeats
    N = args.words
    import torch
    from jlm_amd import generate as G
    from jlm_amd.model import sample
    out = {"bench": "generate", "device": torch.cuda.get_device_name(0), "words_per_row": N}
    for name in ("mid-vtable", "mid-tied"):
        _d, model = _model(root, name)
        m = model.dev
        res = out[name] = {"V": m.V}
        gen = G.Generator(m)
        for R in (256, 1024, 2560):
            prompts = [[G.EOS_ID]] * R
            t = _median_time(lambda: model.generate(prompts, N, seed=1), reps)
            gen.run([np.array([G.EOS_ID])] * R, np.arange(R, dtype=np.int32), N, 1.0, 1, timed=True)
            ms = gen.last_frame_ms                      # [frames, 4]: LSTM step, T projection, logit GEMMs, draw
            med = np.median(ms, axis=0)
            tot = float(med.sum())
            res["rows_%d" % R] = {"tokens": R * N, "s": round(t, 5), "tokens_per_s": round(R * N / t, 1),
                                  "frame_us": {"lstm": round(float(med[0]) * 1e3, 2), "t_proj": round(float(med[1]) * 1e3, 2),
                                               "logit_gemm": round(float(med[2]) * 1e3, 2), "draw": round(float(med[3]) * 1e3, 2),
                                               "total": round(tot * 1e3, 2)},
                                  "logit_gemm_frac": round(float(med[2]) / tot, 4), "draw_frac": round(float(med[3]) / tot, 4),
                                  "tokens_per_s_from_events": round(R / (tot * 1e-3), 1)}
            if R == 2560 or (R == 256 and name == "mid-vtable"):
                trunc = res["rows_%d" % R]["truncated_frame_us"] = {}
                for label, k, p in (("none", None, None), ("top_k_40", 40, None), ("top_p_0.9", None, 0.9), ("top_k_40_top_p_0.9", 40, 0.9)):
                    draws = []
                    for _ in range(reps):
                        gen.run([np.array([G.EOS_ID])] * R, np.arange(R, dtype=np.int32), N, 1.0, 1, timed=True, top_k=k, top_p=p)
                        draws.append(np.median(gen.last_frame_ms, axis=0))
                    med = np.median(draws, axis=0)
                    trunc[label] = {"logit_gemm": round(float(med[2]) * 1e3, 2), "draw": round(float(med[3]) * 1e3, 2),
                                    "draw_min_max": [round(float(np.min(draws, axis=0)[3]) * 1e3, 2), round(float(np.max(draws, axis=0)[3]) * 1e3, 2)],
                                    "total": round(float(med.sum()) * 1e3, 2)}
        if name == "mid-vtable":
            # the host loop it replaces: model.main's predict() + sample() per word, one row
            n_host = 10 if args.quick else 50
            model.hidden = np.zeros((1, m.H))
            model.cell = np.zeros((1, m.H))
            w = G.EOS_ID
            model.predict([w])
            t0 = time.perf_counter()
            for _ in range(n_host):
                pred = model.predict([w])[0]
                w = sample(pred[0])
            t = time.perf_counter() - t0
            res["host_predict_sample_1_row"] = {"tokens": n_host, "s": round(t, 4), "tokens_per_s": round(n_host / t, 1)}
        del model, m, gen
        torch.cuda.empty_cache()
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
