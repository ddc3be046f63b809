"""What the continuous cache costs beside scoring: the time of a score_streams_cached call, of its cache pass alone, and of
score_streams on the same input, in the same process.

  model         mid-tied of tools/rank_bench.py (V = 50 000, H = 512, E = 256), Glorot weights, self-normalised
  shape         B = 128 streams in chunks of n = 20 steps, as python -m jlm_amd.perplexity --mode stream cuts them; N in {500, 2000};
                one value of theta.  Every timed call carries a FULL cache: the streams are first run for N steps.
  whole call    a region = CHUNKS calls behind a synchronise, host clock, state (and cache) carried; score_streams and
                score_streams_cached alternate, REGIONS regions each after a warm-up region of each; the median region is
                reported, with the fastest and the slowest, as milliseconds per call
  cache pass    jlm_cache_rows alone on the rings of such a call (the entry point the op calls behind its last step), device events
                around LAUNCHES launches, median of REPEATS; beside it the bytes it has to read once -- B (N + n) H 4 of state rows
                -- and the rate that makes

One JSON object on stdout and in --out.  Needs a GPU: there is no CPU path.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tools.rank_bench import build_model  # noqa: E402

NUM_STEPS = 20


def region(call, x, y, chunks, torch, carry):
    """`chunks` calls of NUM_STEPS steps, what `carry` holds carried and returned; -> (seconds, carry)"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(chunks):
        cols = slice(i * NUM_STEPS, (i + 1) * NUM_STEPS)
        carry = call(x[:, cols], y[:, cols], carry)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, carry


def cache_pass_ms(m, spec, state, B, torch, launches, repeats):
    """jlm_cache_rows alone over the rings of a call of NUM_STEPS steps that carries `state`"""
    from jlm_amd import _lib
    from jlm_amd.cache import Rings
    rings = Rings(m, spec, B, NUM_STEPS, [NUM_STEPS] * B, state)
    k = rings.carried
    # the call's own steps: any existing states and words will do for a timing (the carried ones, again)
    rings.hist[k:k + NUM_STEPS].copy_(rings.hist[:NUM_STEPS])
    rings.words[k:k + NUM_STEPS].copy_(rings.words[:NUM_STEPS])
    th = (ctypes.c_float * 1)(spec.theta)
    lib = _lib.lib()

    def launch():
        rc = lib.jlm_cache_rows(rings.hist.data_ptr(), rings.words.data_ptr(), rings.cap, B, m.H, int(bool(m.split_lstm)), float(m.h_scale or 1.0),
                                k, NUM_STEPS, rings.first.data_ptr(), rings.len.data_ptr(), spec.size, th, 1, rings.lpc.data_ptr(),
                                rings.flags.data_ptr(), None)
        if rc:
            raise SystemExit("jlm_cache_rows failed with code %d" % rc)

    launch()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _i in range(launches):
            launch()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / launches)
    return sorted(out), k


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=128)
    ap.add_argument("--sizes", type=int, nargs="+", default=[500, 2000])
    ap.add_argument("--theta", type=float, default=0.3)
    ap.add_argument("--chunks", type=int, default=10, help="calls of 20 steps per timed region")
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON object here")
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("cache_bench needs a GPU: a CPU run measures nothing")
    from jlm_amd.cache import CacheSpec
    model = build_model("mid-tied")
    m = model.dev
    B, V = args.rows, m.V
    out = {"model": "mid-tied", "H": m.H, "V": V, "rows": B, "num_steps": NUM_STEPS, "chunks_per_region": args.chunks,
           "regions": args.regions, "state_rows": "split f16" if m.split_lstm else "f32"}
    rng = np.random.RandomState(B)
    stream = rng.randint(0, V, size=(B, args.chunks * NUM_STEPS + 1)).astype(np.int32)
    x, y = stream[:, :-1], stream[:, 1:]

    def plain(a, b, carry):
        _nll, h, c = model.score_streams(a, b, *(carry or (None, None)))
        return h, c

    for N in args.sizes:
        spec = CacheSpec(N, args.theta, 0.1)
        fill = rng.randint(0, V, size=(B, N + 1)).astype(np.int32)
        full = model.score_streams_cached(fill[:, :-1], fill[:, 1:], spec)              # N steps: every stream's cache is full
        start = (full.h, full.c, full.state)

        def cached(a, b, carry):
            res = model.score_streams_cached(a, b, spec, *carry)
            return res.h, res.c, res.state

        region(plain, x, y, 2, torch, None)
        region(cached, x, y, 2, torch, start)
        secs = {"score_streams": [], "score_streams_cached": []}
        for _ in range(args.regions):
            secs["score_streams"].append(region(plain, x, y, args.chunks, torch, None)[0])
            secs["score_streams_cached"].append(region(cached, x, y, args.chunks, torch, start)[0])
        res = {}
        for k, s in secs.items():
            s = sorted(s)
            res[k + "_ms_per_call"] = [round(1e3 * v / args.chunks, 4) for v in (s[0], s[len(s) // 2], s[-1])]
        ms, carried = cache_pass_ms(m, spec, full.state, B, torch, args.launches, args.repeats)
        nbytes = B * (carried + NUM_STEPS) * m.H * 4
        med = ms[len(ms) // 2]
        res["cache_pass_ms"] = [round(ms[0], 4), round(med, 4), round(ms[-1], 4)]
        res["cache_pass_state_bytes"] = nbytes
        res["cache_pass_GBps"] = round(nbytes / (med * 1e-3) / 1e9, 1)
        res["cache_pass_share_of_call"] = round(med / res["score_streams_cached_ms_per_call"][1], 4)
        res["call_ratio_cached_over_plain"] = round(res["score_streams_cached_ms_per_call"][1] / res["score_streams_ms_per_call"][1], 4)
        out["N=%d" % N] = res
        print(N, json.dumps(res), file=sys.stderr, flush=True)
        del full, start
        torch.cuda.empty_cache()
    text = json.dumps(out)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return out


if __name__ == "__main__":
    main()
