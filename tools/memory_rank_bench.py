"""What ranking under a memory costs: tokens/s of LSTM_Model.rank_streams and rank_streams_memory in the same process, where a step's
time goes, and what one predict_next_memory call takes.

  model         mid-tied of tools/rank_bench.py (V = 50 000, H = 512, E = 256, Glorot weights, self-normalised)
  rows, steps   B streams (64 and 1 024) in chunks of 20 steps, the state carried from chunk to chunk
  memory        N = 10^4 / 10^5 / 10^6 entries: the states of one warm-up chunk, repeated up to N entries (what a key holds does not
                change what reading it costs; the repeats make ties, which the select resolves by index as it must), words at random
  mixture       K = 64 and 1 024, theta 0.3, lam 0.1
  timing        tools/rank_cache_bench.py's regions: CHUNKS chunks of one driver behind a synchronise, host clock; the drivers
                alternate, REGIONS regions each after a warm-up region of each; the median region with the fastest and the slowest
  split         the event brackets of one timed chunk under the memory (LSTM step, T projection, logit GEMMs, retrieval, patch,
                ranking), median over its steps.  The retrieval's bracket holds both of its kernels, chunk after chunk: its score and
                select parts are NOT separated here (that takes a kernel trace in a run of its own)
  predict       predict_next_memory at 1 and 64 rows: median of CALLS calls, each behind a synchronise

One JSON object on stdout and in --out.  Needs a GPU: there is no CPU path.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tools.rank_bench import NUM_STEPS, build_model      # noqa: E402
from tools.rank_cache_bench import region                 # noqa: E402


def big_memory(m, x, y, N, torch):
    """a memory of N entries: one chunk's states repeated"""
    from jlm_amd.memory import Memory
    base = Memory.build(m, x[:, :NUM_STEPS], y[:, :NUM_STEPS], NUM_STEPS)
    reps = -(-N // base.N)
    keys = base.keys.repeat(reps, 1)[:N].contiguous()
    words = torch.from_numpy(np.random.RandomState(N).randint(0, m.dev.V, size=N).astype(np.int32)).to(keys.device)
    return Memory(m.dev, keys, words)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--sizes", type=int, nargs="+", default=[10 ** 4, 10 ** 5, 10 ** 6])
    ap.add_argument("--ks", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--chunks", type=int, default=2, help="chunks of 20 steps per timed region")
    ap.add_argument("--regions", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10, help="predict_next_memory calls per figure")
    ap.add_argument("--model", default="mid-tied")
    ap.add_argument("--out", default=None, help="also write the JSON object here")
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("memory_rank_bench needs a GPU: a CPU run measures nothing")
    from jlm_amd.memory import MemoryMix, MixBuffers, RetrievalBuffers
    m = build_model(args.model)
    V = m.dev.V
    index = m.reading_index()
    out = {"model": args.model, "num_steps": NUM_STEPS, "chunks_per_region": args.chunks, "regions": args.regions}
    for B in args.rows:
        rng = np.random.RandomState(B)
        stream = rng.randint(0, V, size=(B, args.chunks * NUM_STEPS + 1)).astype(np.int32)
        x, y = stream[:, :-1], stream[:, 1:]
        for N in args.sizes:
            memory = big_memory(m, x[:64], y[:64], N, torch)
            for K in args.ks:
                mix = MemoryMix(memory, 0.3, 0.1, K)

                def plain(a, b, carry):
                    _r, h, c = m.rank_streams(a, b, carry[0], carry[1])
                    return h, c

                def under(a, b, carry):
                    res = m.rank_streams_memory(a, b, mix, carry[0], carry[1])
                    return res.h, res.c

                drivers = {"rank_streams": plain, "rank_streams_memory": under}
                secs = {k: [] for k in drivers}
                for k, fn in drivers.items():
                    region(fn, x, y, 1, (None, None), torch)                     # warm-up: every shape of the timed window
                for _ in range(args.regions):
                    for k, fn in drivers.items():                                # alternating
                        secs[k].append(region(fn, x, y, args.chunks, (None, None), torch))
                tokens = B * args.chunks * NUM_STEPS
                res = {"chunk_keys": RetrievalBuffers.chunk_keys(N, B)}
                for k, s in secs.items():
                    s = sorted(s)
                    res[k] = {"tokens_per_s": round(tokens / s[len(s) // 2]), "region_s": [round(s[0], 4), round(s[len(s) // 2], 4), round(s[-1], 4)]}
                rk = m._ranker()
                buf = MixBuffers(m.dev, mix, B, NUM_STEPS)
                rk.run(x[:, :NUM_STEPS].T, y[:, :NUM_STEPS].T, [B] * NUM_STEPS, levels=rk.levels(index, 8), timed=True, rings=buf)
                ms = np.median(rk.last_step_ms, axis=0)
                res["step_ms"] = dict(zip(("lstm_step", "t_projection", "logit_gemms", "retrieval", "patch", "ranking"),
                                          [round(float(v), 4) for v in ms]))
                flops = 2.0 * B * N * m.dev.H
                res["retrieval"] = {"product_flops": flops, "score_bytes_written": 4 * B * N,
                                    "TFLOPs_if_all_products": round(flops / (float(ms[3]) * 1e-3) / 1e12, 2)}
                del buf
                if B == args.rows[0]:
                    for rows in (1, 64):
                        hh = memory.keys[:rows].contiguous()
                        t = []
                        for _ in range(args.calls + 2):
                            torch.cuda.synchronize()
                            t0 = time.perf_counter()
                            m.predict_next_memory(hh, mix, n=10)
                            torch.cuda.synchronize()
                            t.append(time.perf_counter() - t0)
                        t = sorted(t[2:])
                        res["predict_next_memory rows=%d" % rows] = {"ms": [round(1e3 * t[0], 3), round(1e3 * t[len(t) // 2], 3), round(1e3 * t[-1], 3)]}
                out["B=%d N=%d K=%d" % (B, N, K)] = res
                print(B, N, K, json.dumps(res), file=sys.stderr, flush=True)
                if args.out:                                                   # (kept as far as it got)
                    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                    with open(args.out, "w") as f:
                        f.write(json.dumps(out, indent=1) + "\n")
            del memory
            torch.cuda.empty_cache()
    text = json.dumps(out, indent=1)
    print(text)
    return out


if __name__ == "__main__":
    main()
