"""What scoring against a memory of hidden states costs beside scoring: the time of a score_streams_memory call, of its memory pass
alone, and of score_streams on the same input, in the same process.

  model         mid-tied of tools/rank_bench.py (V = 50 000, H = 512, E = 256), Glorot weights, self-normalised, split rows
  shape         B = 128 streams in calls of n = 20 steps (2 560 queries a call), as python -m jlm_amd.perplexity --mode stream cuts
                them; N in {10^4, 10^5, 10^6} entries; one value of theta.  The memory's keys are state rows the scorer wrote (a few
                thousand of them, repeated up to N: the pass reads N rows whatever they hold), its words random ids.
  whole call    a region = CHUNKS calls behind a synchronise, host clock, state carried; score_streams and score_streams_memory
                alternate, REGIONS regions each after a warm-up region of each; the median region is reported, with the fastest and
                the slowest, as milliseconds per call
  memory pass   jlm_memory_rows alone on the buffers of such a call (the entry point the op calls behind its last step), device
                events around LAUNCHES launches, median of REPEATS with fastest and slowest; beside it the algorithmic matrix rate
                2 Q N H / time against the three-pass f16 ceiling of DESIGN.md 4.1 (838.9 TFLOP/s: split rows issue three
                instructions per product), and the key bytes per second N H 4 / time -- the memory read ONCE; what the pass pulls
                through L2 is that times the query blocks that miss

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
CEILING_TFLOPS = 838.9


def region(call, x, y, chunks, torch):
    """`chunks` calls of NUM_STEPS steps, the state carried; -> seconds"""
    carry = (None, None)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(chunks):
        cols = slice(i * NUM_STEPS, (i + 1) * NUM_STEPS)
        carry = call(x[:, cols], y[:, cols], carry)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def memory_pass_ms(m, memory, spec, B, torch, launches, repeats):
    """jlm_memory_rows alone over the buffers of a call of NUM_STEPS steps: the queries are the memory's first B * NUM_STEPS rows"""
    from jlm_amd import _lib
    from jlm_amd.memory import MemoryRings
    rings = MemoryRings(m, memory, spec, B, NUM_STEPS, [NUM_STEPS] * B)
    Q = B * NUM_STEPS
    rings.q_rows.view(Q, m.H).copy_(memory.keys[:Q])
    rings.q_words.view(Q).copy_(memory.words[:Q])
    th = (ctypes.c_float * 1)(spec.theta)
    lib = _lib.lib()

    def launch():
        rc = lib.jlm_memory_rows(memory.keys.data_ptr(), memory.words.data_ptr(), memory.N, m.H, int(memory.split), memory.h_scale,
                                 rings.q_rows.data_ptr(), rings.q_words.data_ptr(), B, NUM_STEPS, rings.len.data_ptr(), th, 1,
                                 rings.lpm.data_ptr(), rings.workspace.data_ptr(), rings.workspace.numel() * 4, rings.flags.data_ptr(), None)
        if rc:
            raise SystemExit("jlm_memory_rows failed with code %d" % rc)

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
    return sorted(out)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=128)
    ap.add_argument("--sizes", type=int, nargs="+", default=[10 ** 4, 10 ** 5, 10 ** 6])
    ap.add_argument("--theta", type=float, default=0.3)
    ap.add_argument("--chunks", type=int, default=5, help="calls of 20 steps per timed region")
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--launches", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON object here")
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("memory_bench needs a GPU: a CPU run measures nothing")
    from jlm_amd.memory import Memory, MemorySpec, keys_per_split
    model = build_model("mid-tied")
    m = model.dev
    B, V = args.rows, m.V
    out = {"model": "mid-tied", "H": m.H, "V": V, "rows": B, "num_steps": NUM_STEPS, "queries": B * NUM_STEPS, "chunks_per_region": args.chunks,
           "regions": args.regions, "state_rows": "split f16" if m.split_lstm else "f32", "ceiling_TFLOPs": CEILING_TFLOPS}
    rng = np.random.RandomState(B)
    stream = rng.randint(0, V, size=(B, args.chunks * NUM_STEPS + 1)).astype(np.int32)
    x, y = stream[:, :-1], stream[:, 1:]
    seed = Memory.build(model, x, y, NUM_STEPS)                                            # B * chunks * 20 real state rows
    spec = MemorySpec(args.theta, 0.1)

    def plain(a, b, carry):
        _nll, h, c = model.score_streams(a, b, *carry)
        return h, c

    for N in args.sizes:
        reps = -(-N // seed.N)
        with m._ctx():
            keys = seed.keys.repeat(reps, 1)[:N].contiguous()
            words = torch.from_numpy(rng.randint(0, V, size=N).astype(np.int32)).to(m.device)
        memory = Memory(m, keys, words)

        def against(a, b, carry):
            res = model.score_streams_memory(a, b, memory, spec, *carry)
            return res.h, res.c

        region(plain, x, y, 2, torch)
        region(against, x, y, 2, torch)
        secs = {"score_streams": [], "score_streams_memory": []}
        for _ in range(args.regions):
            secs["score_streams"].append(region(plain, x, y, args.chunks, torch))
            secs["score_streams_memory"].append(region(against, x, y, args.chunks, torch))
        res = {"keys_per_split": keys_per_split(N), "splits": -(-N // keys_per_split(N))}
        for k, s in secs.items():
            s = sorted(s)
            res[k + "_ms_per_call"] = [round(1e3 * v / args.chunks, 4) for v in (s[0], s[len(s) // 2], s[-1])]
        ms = memory_pass_ms(m, memory, spec, B, torch, args.launches, args.repeats)
        med = ms[len(ms) // 2]
        Q = B * NUM_STEPS
        res["memory_pass_ms"] = [round(ms[0], 4), round(med, 4), round(ms[-1], 4)]
        res["memory_pass_TFLOPs"] = round(2.0 * Q * N * m.H / (med * 1e-3) / 1e12, 2)
        res["memory_pass_share_of_ceiling"] = round(res["memory_pass_TFLOPs"] / CEILING_TFLOPS, 4)
        res["key_bytes"] = N * m.H * 4
        res["key_GBps"] = round(N * m.H * 4 / (med * 1e-3) / 1e9, 1)
        res["memory_pass_share_of_call"] = round(med / res["score_streams_memory_ms_per_call"][1], 4)
        res["call_ratio_memory_over_plain"] = round(res["score_streams_memory_ms_per_call"][1] / res["score_streams_ms_per_call"][1], 4)
        out["N=%d" % N] = res
        print(N, json.dumps(res), file=sys.stderr, flush=True)
        del memory, keys, words
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
