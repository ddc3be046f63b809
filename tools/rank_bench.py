"""What ranking costs beside scoring: tokens/s of LSTM_Model.rank_streams and score_streams in the same process, and where a
ranking step's time goes.

  models        mid-tied and mid-vtable of tools/train_bench.py (V = 50 000, H = 512; E = 256 / segments 200, 100, 50), Glorot
                weights, self-normalised; readings from the synthetic lexicon (1 .. 4 kana over 80)
  rows, steps   as python -m jlm_amd.perplexity --mode stream uses them: B streams (its default 64, and 1 024) in chunks of 20 steps,
                the state carried from chunk to chunk
  timing        a region = CHUNKS chunks of one driver behind a synchronise, host clock; the two drivers alternate, REGIONS regions
                each after a warm-up region of each; the median region is reported, with the fastest and the slowest
  split         the event brackets of one timed ranking chunk (LSTM step, T projection, logit GEMMs, ranking), median over its steps
  bound         the counting launch reads rows x V x 4 bytes of logits once, plus the gathers (the words with a reading, once more,
                and 4 bytes of index each): the time that takes at the measured rate is printed beside the HBM figure of
                the data sheet so the two can be compared

One JSON object on stdout and in --out.  Needs a GPU: there is no CPU path.
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

NUM_STEPS = 20
HBM_BYTES_PER_S = 8.0e12            # the HBM3E peak of the MI355X data sheet (about 6.3e12 is what a float4 copy reaches)


def build_model(name):
    from jlm_amd import config as jconfig, synth, train as T
    mode = name.split("-")[1]
    cfg = synth.make_config(50000, 512, 256, mode, synth.README_SEGS, True)
    root = tempfile.mkdtemp(prefix="jlm_rank_bench_")
    synth.write_lexicon(root, cfg["vocab_size"])
    jconfig.set_root(root)
    T.write_experiment(1, cfg, T.init_weights(cfg, None, 101))
    from jlm_amd.model import LSTM_Model
    return LSTM_Model(experiment_id=1)


def region(fn, x, y, chunks, torch):
    """`chunks` chunks of NUM_STEPS steps through fn(inputs, targets, h, c) -> (_, h, c), the state carried; -> seconds"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    h = c = None
    for i in range(chunks):
        cols = slice(i * NUM_STEPS, (i + 1) * NUM_STEPS)
        _out, h, c = fn(x[:, cols], y[:, cols], h, c)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--chunks", type=int, default=8, help="chunks of 20 steps per timed region")
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--models", nargs="+", default=["mid-tied", "mid-vtable"])
    ap.add_argument("--out", default=None, help="also write the JSON object here")
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("rank_bench needs a GPU: a CPU run measures nothing")
    out = {"num_steps": NUM_STEPS, "chunks_per_region": args.chunks, "regions": args.regions}
    for name in args.models:
        m = build_model(name)
        V = m.dev.V
        index = m.reading_index()
        n_read = len(index)
        for B in args.rows:
            rng = np.random.RandomState(B)
            stream = rng.randint(0, V, size=(B, args.chunks * NUM_STEPS + 1)).astype(np.int32)
            x, y = stream[:, :-1], stream[:, 1:]
            drivers = {"score_streams": m.score_streams, "rank_streams": m.rank_streams,
                       "rank_streams(readings=False)": lambda a, b, h, c: m.rank_streams(a, b, h, c, readings=False)}
            secs = {k: [] for k in drivers}
            for k, fn in drivers.items():
                region(fn, x, y, 2, torch)                                   # warm-up: every shape of the timed window
            for _ in range(args.regions):
                for k, fn in drivers.items():                                # alternating
                    secs[k].append(region(fn, x, y, args.chunks, torch))
            tokens = B * args.chunks * NUM_STEPS
            res = {}
            for k, s in secs.items():
                s = sorted(s)
                res[k] = {"tokens_per_s": round(tokens / s[len(s) // 2]), "region_s": [round(s[0], 4), round(s[len(s) // 2], 4), round(s[-1], 4)]}
            # the event brackets of one chunk
            rk = m._ranker()
            lv = rk.levels(index, 8)
            rk.run(x[:, :NUM_STEPS].T, y[:, :NUM_STEPS].T, [B] * NUM_STEPS, levels=lv, timed=True)
            ms = np.median(rk.last_step_ms, axis=0)
            res["rank_step_ms"] = dict(zip(("lstm_step", "t_projection", "logit_gemms", "ranking"), [round(float(v), 4) for v in ms]))
            sc = m._scorer()
            sc.run(x[:, :NUM_STEPS].T, y[:, :NUM_STEPS].T, [B] * NUM_STEPS, timed=True)
            ms_s = np.median(sc.last_step_ms, axis=0)
            res["score_step_ms"] = dict(zip(("lstm_step", "t_projection", "normaliser", "fold"), [round(float(v), 4) for v in ms_s]))
            # what the counting launch has to move: the row once, then per word with a reading its index and its logit again (level 0);
            # the deeper levels add about 1 / 80 of that a level
            scan, gather = B * V * 4, B * n_read * 8
            t_rank = float(ms[3]) * 1e-3
            res["ranking_launch"] = {"scan_bytes": scan, "gather_bytes": gather, "ms": round(float(ms[3]), 4),
                                     "achieved_GBps_scan_only": round(scan / t_rank / 1e9, 1),
                                     "achieved_GBps_scan_and_gather": round((scan + gather) / t_rank / 1e9, 1),
                                     "ms_at_hbm_peak_scan_only": round(scan / HBM_BYTES_PER_S * 1e3, 4)}
            out["%s B=%d" % (name, B)] = res
            print(name, B, json.dumps(res), file=sys.stderr, flush=True)
        del m
        torch.cuda.empty_cache()
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return out


if __name__ == "__main__":
    main()
