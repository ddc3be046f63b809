"""What the n-gram mixture costs on the ranking and prediction side: tokens/s of LSTM_Model.rank_streams and rank_streams_ngram in the
same process, where a mixed ranking step's time goes, what predict_top takes with and without a table, and -- beside the argument
that their launches are identical by construction -- the plain rank_streams and complete legs of this build against another build's.

  model         mid-tied of tools/rank_bench.py (V = 50 000, H = 512, E = 256, Glorot weights, self-normalised)
  rows, steps   B streams (64 and 1 024) in chunks of 20 steps, the state and the last two words carried from chunk to chunk
  tables        synthetic, about 10^5 and 10^6 entries, orders 2 and 3: a unigram for every word; bigrams (v, w) and, at order 3,
                trigrams (u, v, w) whose contexts are drawn from the stream's own (u, v) pairs with random successors, half of the
                bigrams with a back-off weight -- so every timed row resolves a bigram list and most of them a trigram context
  timing        tools/rank_bench.py's regions: CHUNKS chunks of one driver behind a synchronise, host clock; the drivers alternate,
                REGIONS regions each after a warm-up region of each; the median region with the fastest and the slowest
  split         the event brackets of one timed mixed chunk (LSTM step, T projection, logit GEMMs, n-gram patch, ranking), median
                over its steps: the patch launch alone, by device events.  It reads and writes rows x V x 4 bytes of logits and reads
                V x 4 bytes of unigrams per row (from cache): the rate it reaches is printed beside the HBM figure of the data sheet
  predict       predict_top at 1 and 64 contexts with and without the largest table: median of CALLS calls, each behind a synchronise
  --against DIR another checkout of the project, BUILT (its parent commit, say): the plain legs -- rank_streams at the first row count
                and complete at 16 prompts x beam 10 x 5 words -- run in fresh child processes, this tree and DIR alternating, ROUNDS
                times (the side that goes first alternates too); every process's median, sorted, of each side

One JSON object on stdout and in --out.  Needs a GPU: there is no CPU path.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.environ.get("JLM_BENCH_REPO") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tools.rank_bench import HBM_BYTES_PER_S, NUM_STEPS, build_model      # noqa: E402


def synthetic_table(x, V, n_entries, order, seed=0):
    """an NGramTable of about ``n_entries`` entries (module docstring) for the streams x [B, n]"""
    from jlm_amd.ngram import NGramTable
    rng = np.random.RandomState(seed)
    keys = [np.arange(1, V + 1, dtype=np.int64)]
    lp = [-rng.uniform(2.0, 14.0, size=V)]
    bow = [np.where(rng.rand(V) < 0.5, -rng.uniform(0.0, 2.0, size=V), 0.0)]
    rest = max(n_entries - V, 0)
    n_bi = rest if order == 2 else rest // 2
    n_tri = rest - n_bi if order == 3 else 0
    if order >= 2 and n_bi:
        k2 = np.unique(((rng.randint(0, V, size=n_bi).astype(np.int64) + 1) << 21) | (rng.randint(0, V, size=n_bi).astype(np.int64) + 1))
        keys.append(k2)
        lp.append(-rng.uniform(0.1, 9.0, size=k2.size))
        bow.append(np.where(rng.rand(k2.size) < 0.5, -rng.uniform(0.0, 2.0, size=k2.size), 0.0))
    if n_tri:
        at = rng.randint(0, x.shape[1] - 1, size=n_tri)
        row = rng.randint(0, x.shape[0], size=n_tri)
        u, v = x[row, at].astype(np.int64), x[row, at + 1].astype(np.int64)
        k3 = np.unique(((u + 1) << 42) | ((v + 1) << 21) | (rng.randint(0, V, size=n_tri).astype(np.int64) + 1))
        keys.append(k3)
        lp.append(-rng.uniform(0.1, 6.0, size=k3.size))
        bow.append(np.zeros(k3.size))
    return NGramTable(np.concatenate(keys), np.concatenate(lp), np.concatenate(bow), order)


def region(step, x, y, chunks, carry, torch):
    """`chunks` chunks of NUM_STEPS steps through step(inputs, targets, carry) -> carry; -> seconds"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(chunks):
        cols = slice(i * NUM_STEPS, (i + 1) * NUM_STEPS)
        carry = step(x[:, cols], y[:, cols], carry)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def three(s):
    s = sorted(s)
    return [round(s[0], 4), round(s[len(s) // 2], 4), round(s[-1], 4)]


def calls_ms(fn, calls, torch):
    t = []
    for _ in range(calls + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append(1e3 * (time.perf_counter() - t0))
    return three(t[2:])


def plain_legs(args):
    """the child of --against: the plain legs of the tree it was started in -> one JSON line"""
    import torch
    m = build_model(args.model)
    V = m.dev.V
    B = args.rows[0]
    rng = np.random.RandomState(B)
    stream = rng.randint(0, V, size=(B, args.chunks * NUM_STEPS + 1)).astype(np.int32)
    x, y = stream[:, :-1], stream[:, 1:]

    def plain(a, b, carry):
        _r, h, c = m.rank_streams(a, b, carry[0], carry[1], readings=False)
        return h, c
    region(plain, x, y, 2, (None, None), torch)
    secs = [region(plain, x, y, args.chunks, (None, None), torch) for _ in range(args.regions)]
    prompts = [[1] + [int(w) for w in rng.randint(2, V, size=3)] for _ in range(16)]
    out = {"rank_streams_tokens_per_s": round(B * args.chunks * NUM_STEPS / sorted(secs)[len(secs) // 2]),
           "complete_ms": calls_ms(lambda: m.complete(prompts, 5, beam_width=10), args.calls, torch)}
    print("LEGS " + json.dumps(out))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--entries", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--orders", type=int, nargs="+", default=[2, 3])
    ap.add_argument("--chunks", type=int, default=4, help="chunks of 20 steps per timed region")
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20, help="predict_top / complete calls per figure")
    ap.add_argument("--model", default="mid-tied")
    ap.add_argument("--against", default=None, metavar="DIR", help="a built checkout to alternate the plain legs with")
    ap.add_argument("--rounds", type=int, default=3, help="--against: child processes per side")
    ap.add_argument("--legs", action="store_true", help="(the child of --against)")
    ap.add_argument("--out", default=None, help="also write the JSON object here")
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("rank_ngram_bench needs a GPU: a CPU run measures nothing")
    if args.legs:
        return plain_legs(args)
    from jlm_amd.ngram import NGramMix
    from jlm_amd.ngram_mix import NgramPatch, forced_hist
    m = build_model(args.model)
    V = m.dev.V
    out = {"model": args.model, "num_steps": NUM_STEPS, "chunks_per_region": args.chunks, "regions": args.regions}
    last_mix = None
    for B in args.rows:
        rng = np.random.RandomState(B)
        stream = rng.randint(0, V, size=(B, args.chunks * NUM_STEPS + 1)).astype(np.int32)
        x, y = stream[:, :-1], stream[:, 1:]
        for n_entries in args.entries:
            for order in args.orders:
                t0 = time.perf_counter()
                mix = NGramMix(synthetic_table(x, V, n_entries, order), 0.3)
                arr = mix.table.successor_arrays(V)
                build_s = time.perf_counter() - t0
                last_mix = mix

                def plain(a, b, carry):
                    _r, h, c = m.rank_streams(a, b, carry[0], carry[1])
                    return h, c, None

                def mixed(a, b, carry):
                    res = m.rank_streams_ngram(a, b, mix, carry[0], carry[1], carry[2])
                    return res.h, res.c, res.tail

                drivers = {"rank_streams": plain, "rank_streams_ngram": mixed}
                secs = {k: [] for k in drivers}
                for k, fn in drivers.items():
                    region(fn, x, y, 2, (None, None, None), torch)           # warm-up: every shape of the timed window, the table's upload
                for _ in range(args.regions):
                    for k, fn in drivers.items():                            # alternating
                        secs[k].append(region(fn, x, y, args.chunks, (None, None, None), torch))
                tokens = B * args.chunks * NUM_STEPS
                res = {"entries": len(mix.table), "contexts": int(arr["n_ctx"]), "max_probe": int(arr["max_probe"]),
                       "table_build_s": round(build_s, 2)}
                for k, s in secs.items():
                    res[k] = {"tokens_per_s": round(tokens / sorted(s)[len(s) // 2]), "region_s": three(s)}
                # the event brackets of one mixed chunk
                rk = m._ranker()
                patch = NgramPatch(m.dev, mix, forced_hist(x[:, :NUM_STEPS].T))
                rk.run(x[:, :NUM_STEPS].T, y[:, :NUM_STEPS].T, [B] * NUM_STEPS, levels=rk.levels(m.reading_index(), 8), timed=True, rings=patch)
                ms = np.median(rk.last_step_ms, axis=0)
                res["mixed_step_ms"] = dict(zip(("lstm_step", "t_projection", "logit_gemms", "ngram_patch", "ranking"),
                                                [round(float(v), 4) for v in ms]))
                p_bytes = B * V * 4 * 2
                res["patch_launch"] = {"logit_bytes": p_bytes, "ms": round(float(ms[3]), 4),
                                       "achieved_GBps": round(p_bytes / (float(ms[3]) * 1e-3) / 1e9, 1),
                                       "ms_at_hbm_peak": round(p_bytes / HBM_BYTES_PER_S * 1e3, 4)}
                out["B=%d entries=%d order=%d" % (B, n_entries, order)] = res
                print(B, n_entries, order, json.dumps(res), file=sys.stderr, flush=True)
                torch.cuda.empty_cache()
    rng = np.random.RandomState(1)
    for rows in (1, 64):
        contexts = [[1] + [int(w) for w in rng.randint(2, V, size=3)] for _ in range(rows)]
        out["predict_top rows=%d" % rows] = {"ms": calls_ms(lambda: m.predict_top(contexts, n=10), args.calls, torch),
                                             "ms_with_table": calls_ms(lambda: m.predict_top(contexts, n=10, ngram=last_mix), args.calls, torch)}
    if args.against:
        here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        sides = {"this": here, "against": os.path.abspath(args.against)}
        legs = {k: [] for k in sides}
        for i in range(args.rounds):
            for k, root in list(sides.items())[::1 if i % 2 == 0 else -1]:   # alternating, the first side too; a fresh process each
                env = dict(os.environ, JLM_BENCH_REPO=root)
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--legs", "--model", args.model, "--rows", str(args.rows[0]),
                                    "--chunks", str(args.chunks), "--regions", str(args.regions), "--calls", str(args.calls)],
                                   cwd=root, env=env, capture_output=True, text=True, timeout=600)
                line = [l for l in r.stdout.splitlines() if l.startswith("LEGS ")]
                if r.returncode != 0 or not line:
                    raise SystemExit("the plain legs failed in %s:\n%s" % (root, r.stderr[-2000:]))
                legs[k].append(json.loads(line[0][5:]))
        out["plain_legs"] = {k: {"rank_streams_tokens_per_s": sorted(v["rank_streams_tokens_per_s"] for v in vs),
                                 "complete_ms_median": sorted(v["complete_ms"][1] for v in vs)} for k, vs in legs.items()}
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return out


if __name__ == "__main__":
    main()
