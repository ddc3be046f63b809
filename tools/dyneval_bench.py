"""Time of a dynamic-evaluation step on the device (jlm_amd.dyneval.DynEvalDeviceStepper, csrc/jlm_train.hip): one JSON line.

  models        mid-tied and mid-vtable (V = 50 000, H = 512; E = 256 / segments 200, 100, 50), Glorot weights
  per (model, B, T) at (1, 5), (1, 20), (4, 20), rule sgd, lr 0.005, lam 0.02 (rms: lr 3e-4, a flat RMS of 1e-3), IN THE SAME RUN:
                split     the module's routing (SPLIT_KC, SPLIT_MAX_TILES, or --kc / --max-tiles): the few-tile, long-contraction
                          products through train_gemm_splitk
                unsplit   split_max_tiles=0: every product is the trainer's train_gemm launch -- what the step was without the split
                tokens/s over 50 timed steps after 10 warm-up steps, the median of three such regions (wall clock around a
                synchronised region; random ids), and milliseconds per phase of a step by HIP events (a run of its own, 10 steps)
  --rms         also the rms rule's step (the update reads a fourth buffer) at the same shapes, split routing

    python tools/dyneval_bench.py [--quick] [--kc N] [--max-tiles N] [--rms] [--out FILE]
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

SHAPES = [(1, 5), (1, 20), (4, 20)]


def _model(name):
    from jlm_amd import synth, train as T
    cfg = synth.make_config(50000, 512, 256, name.split("-")[1], synth.README_SEGS, True)
    return cfg, T.init_weights(cfg, None, 101)


def _batches(V, B, Tn, n, seed=0):
    rng = np.random.RandomState(seed)
    return [(rng.randint(0, V, (B, Tn)), rng.randint(0, V, (B, Tn))) for _ in range(n)]


def _region(st, batches, torch):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for x, y in batches:
        st.step_async(x, y)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def _timed(st, batches, n_warm, torch):
    _region(st, batches[:n_warm], torch)
    secs = sorted(_region(st, batches, torch) for _ in range(3))
    st.losses()
    st.timed = True
    for x, y in batches[:10]:
        st.step_async(x, y)
    ph = {k: round(v / 10, 4) for k, v in st.phase_ms().items()}
    st.timed = False
    return secs, ph


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--quick", action="store_true", help="10 timed steps per region")
    ap.add_argument("--kc", type=int, default=None, help="split_kc instead of the module's SPLIT_KC")
    ap.add_argument("--max-tiles", type=int, default=None, dest="max_tiles", help="split_max_tiles instead of the module's SPLIT_MAX_TILES")
    ap.add_argument("--rms", action="store_true")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args(argv)
    import torch
    from jlm_amd import dyneval as DE, train as T
    n_timed, n_warm = (10, 3) if args.quick else (50, 10)
    kc = DE.SPLIT_KC if args.kc is None else args.kc
    tiles = DE.SPLIT_MAX_TILES if args.max_tiles is None else args.max_tiles
    out = {"bench": "dyneval", "device": torch.cuda.get_device_name(0), "timed_steps": n_timed, "warmup": n_warm, "split_kc": kc,
           "split_max_tiles": tiles}
    for name in ("mid-tied", "mid-vtable"):
        cfg, w = _model(name)
        for B, Tn in SHAPES:
            batches = _batches(50000, B, Tn, n_timed)
            legs = [("split", "sgd", tiles), ("unsplit", "sgd", 0)] + ([("split rms", "rms", tiles)] if args.rms else [])
            row = {}
            for leg, rule, max_tiles in legs:
                stats = T._map(w, lambda a: np.full(np.shape(a), 1e-3, dtype=np.float32)) if rule == "rms" else None
                lr = 0.005 if rule == "sgd" else 3e-4                  # (a flat RMS of 1e-3 beside eps 1e-3: 0.15 g per step)
                st = DE.DynEvalDeviceStepper(cfg, w, DE.DynEvalSpec(lr, 0.02, rule, batch_size=B, num_steps=Tn), stats, split_kc=kc,
                                             split_max_tiles=max_tiles)
                secs, ph = _timed(st, batches, n_warm, torch)
                row[leg] = {"tokens_per_s": round(B * Tn * n_timed / secs[1]), "step_ms": round(secs[1] / n_timed * 1e3, 3),
                            "regions_s": [round(s, 4) for s in secs], "phase_ms": ph, "split_scratch_words": int(st.part.numel())}
                del st
                torch.cuda.empty_cache()
            row["split_over_unsplit"] = round(row["split"]["step_ms"] / row["unsplit"]["step_ms"], 4)
            out["%s B=%d T=%d" % (name, B, Tn)] = row
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return out


if __name__ == "__main__":
    main()
