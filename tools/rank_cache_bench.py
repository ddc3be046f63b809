"""What the continuous cache costs on the ranking side: tokens/s of LSTM_Model.rank_streams and rank_streams_cached in the same
process, where a cached ranking step's time goes, and what one predict_next_cached call takes.

  model         mid-tied of tools/rank_bench.py (V = 50 000, H = 512, E = 256, Glorot weights, self-normalised)
  rows, steps   B streams (64 and 1 024) in chunks of 20 steps, the state and the cache carried from chunk to chunk
  cache         N = 500 and 2 000 entries, FULL from the first timed step: the states of one warm-up chunk, repeated up to N entries
                (what a key holds does not change what reading it costs), theta 0.3, lam 0.1
  timing        tools/rank_bench.py's regions: CHUNKS chunks of one driver behind a synchronise, host clock; the drivers alternate,
                REGIONS regions each after a warm-up region of each; the median region with the fastest and the slowest
  split         the event brackets of one timed cached chunk (LSTM step, T projection, logit GEMMs, cache query, cache patch,
                ranking + ring write), median over its steps; the query launch reads rows x N x H x 4 bytes once: the rate it reaches
                is printed beside the HBM figure of the data sheet
  predict       predict_next_cached at 1 and 64 rows against the full cache: median of CALLS calls, each behind a synchronise

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

from tools.rank_bench import HBM_BYTES_PER_S, NUM_STEPS, build_model      # noqa: E402


def full_state(m, x, y, spec):
    """-> (h, c, a CacheState of spec.size entries): one chunk's states repeated up to the cache's size"""
    from jlm_amd.cache import CacheSpec, CacheState
    res = m.rank_streams_cached(x[:, :NUM_STEPS], y[:, :NUM_STEPS], CacheSpec(NUM_STEPS, spec.theta, spec.lam), readings=False)
    reps = -(-spec.size // NUM_STEPS)
    hist = res.state.hist.repeat(reps, 1, 1)[:spec.size].contiguous()
    words = res.state.words.repeat(reps, 1)[:spec.size].contiguous()
    return res.h, res.c, CacheState(m.dev, hist, words, spec.size)


def region(step, x, y, chunks, carry, torch):
    """`chunks` chunks of NUM_STEPS steps through step(inputs, targets, carry) -> carry; -> seconds"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(chunks):
        cols = slice(i * NUM_STEPS, (i + 1) * NUM_STEPS)
        carry = step(x[:, cols], y[:, cols], carry)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--sizes", type=int, nargs="+", default=[500, 2000])
    ap.add_argument("--chunks", type=int, default=8, help="chunks of 20 steps per timed region")
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20, help="predict_next_cached calls per figure")
    ap.add_argument("--model", default="mid-tied")
    ap.add_argument("--out", default=None, help="also write the JSON object here")
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("rank_cache_bench needs a GPU: a CPU run measures nothing")
    from jlm_amd.cache import CacheSpec, MixRings
    m = build_model(args.model)
    V, H = m.dev.V, m.dev.H
    index = m.reading_index()
    out = {"model": args.model, "num_steps": NUM_STEPS, "chunks_per_region": args.chunks, "regions": args.regions}
    for B in args.rows:
        rng = np.random.RandomState(B)
        stream = rng.randint(0, V, size=(B, args.chunks * NUM_STEPS + 1)).astype(np.int32)
        x, y = stream[:, :-1], stream[:, 1:]
        for N in args.sizes:
            spec = CacheSpec(N, 0.3, 0.1)
            h0, c0, state0 = full_state(m, x, y, spec)

            def plain(a, b, carry):
                _r, h, c = m.rank_streams(a, b, carry[0], carry[1])
                return h, c, None

            def cached(a, b, carry):
                res = m.rank_streams_cached(a, b, spec, carry[0], carry[1], carry[2])
                return res.h, res.c, res.state

            drivers = {"rank_streams": plain, "rank_streams_cached": cached}
            secs = {k: [] for k in drivers}
            for k, fn in drivers.items():
                region(fn, x, y, 2, (h0, c0, state0), torch)                 # warm-up: every shape of the timed window
            for _ in range(args.regions):
                for k, fn in drivers.items():                                # alternating
                    secs[k].append(region(fn, x, y, args.chunks, (h0, c0, state0), torch))
            tokens = B * args.chunks * NUM_STEPS
            res = {}
            for k, s in secs.items():
                s = sorted(s)
                res[k] = {"tokens_per_s": round(tokens / s[len(s) // 2]), "region_s": [round(s[0], 4), round(s[len(s) // 2], 4), round(s[-1], 4)]}
            # the event brackets of one cached chunk
            rk = m._ranker()
            rings = MixRings(m.dev, spec, B, NUM_STEPS, state0)
            rk.run(x[:, :NUM_STEPS].T, y[:, :NUM_STEPS].T, [B] * NUM_STEPS, h=h0, c=c0, levels=rk.levels(index, 8), timed=True, rings=rings)
            ms = np.median(rk.last_step_ms, axis=0)
            res["cached_step_ms"] = dict(zip(("lstm_step", "t_projection", "logit_gemms", "cache_query", "cache_patch", "ranking_and_store"),
                                             [round(float(v), 4) for v in ms]))
            q_bytes = B * N * H * 4
            res["query_launch"] = {"bytes": q_bytes, "ms": round(float(ms[3]), 4), "achieved_GBps": round(q_bytes / (float(ms[3]) * 1e-3) / 1e9, 1),
                                   "ms_at_hbm_peak": round(q_bytes / HBM_BYTES_PER_S * 1e3, 4)}
            del rings
            if B == args.rows[0]:
                for rows in (1, 64):
                    hh, _cc, st = full_state(m, x[:rows], y[:rows], spec)
                    t = []
                    for _ in range(args.calls + 2):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        m.predict_next_cached(hh, st, spec, n=10)
                        torch.cuda.synchronize()
                        t.append(time.perf_counter() - t0)
                    t = sorted(t[2:])
                    res["predict_next_cached rows=%d" % rows] = {"ms": [round(1e3 * t[0], 3), round(1e3 * t[len(t) // 2], 3), round(1e3 * t[-1], 3)]}
            out["B=%d N=%d" % (B, N)] = res
            print(B, N, json.dumps(res), file=sys.stderr, flush=True)
            del state0
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
