"""Cost of decoding under the continuous cache (Decoder.decode_batch(context=CachedContext); csrc/jlm_cache_edge.hip): one JSON object,
printed and written to profiles/decode_cache_bench.json.  Modelled on tools/context_bench.py.

  workload        BASELINE configs[1]: mid-vtable (LSTM h=512, D-softmax* 200/100/50, V = 50 000), 256 sentences x 20 kana, beam 10;
                  a call is `--steps` pipelined 256-sentence steps, strings -> strings (bench.py's timed region)
  legs            no_cache                decode_batch(sentences)                      -- what the parent commit runs
                  context                 decode_batch(sentences, context=<a ContextState primed once>): section 15's reused leg
                  cache_100 / 500 / 2000  decode_batch(sentences, context=<a CachedContext primed once, N words per sentence>)
                  per leg ms per 256-sentence step: median, min and max of `--repeats` calls, the legs alternating call by call so that
                  they see the same machine; before the clock two settle rounds of every leg
  query_bytes     what the query must read per frame, B * n_s * H * 4 bytes (every key once per cell), by shape -- not a measurement
  kernels         cache_cell_query_kernel and cache_cell_patch_kernel ALONE, as jlm_cache_cell_query / jlm_cache_cell_patch launch them
                  for one frame of the workload (256 cells x 10 slots, H = 512 split rows, full windows, 40 list positions a cell of
                  which 8 are words of the window, no normaliser slices) on synthetic operands: device events around 20 back-to-back
                  launches, median of 7 such brackets, ms per launch; the query's achieved bytes/s against query_bytes

    python tools/decode_cache_bench.py [--root DIR] [--steps K] [--repeats N] [--quick] [--out FILE]
    python tools/decode_cache_bench.py --only-plain [--repo CHECKOUT] [--tag NAME]   # the no_cache leg alone, one JSON line; with --repo
                                  the package is imported from another checkout (the parent commit: same launches expected)
    python tools/decode_cache_bench.py --ab-file LINES.jsonl ...                      # embed such lines (interleaved A/B runs) in the result
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (100, 500, 2000)


def _stat(ms):
    return {"median_ms_per_step": round(float(np.median(ms)), 4), "min": round(float(np.min(ms)), 4), "max": round(float(np.max(ms)), 4),
            "calls": len(ms)}


def kernel_events(torch, B, beam, H, N, reps=7, inner=20, J=40, hits=8):
    """ms per launch of the two kernels alone at one frame's shape -> dict"""
    from jlm_amd import _lib
    lib, dev = _lib.lib(), torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator(device="cpu").manual_seed(N)
    rows = lambda *shape: (0.05 * torch.randn(*shape, 2 * H, generator=g)).to(torch.float16).view(torch.float32).to(dev)     # valid split rows
    hist, q = rows(N, B), rows(B * beam)
    words = torch.randint(2, 50000, (N, B), generator=g, dtype=torch.int32).to(dev)
    count = torch.full((B,), N, dtype=torch.int32, device=dev)
    idx = torch.arange(B, dtype=torch.int32, device=dev)
    g0, cnt, slen = idx * beam, torch.full((B,), beam, dtype=torch.int32, device=dev), torch.full((B,), 5, dtype=torch.int32, device=dev)
    wl = torch.randint(2, 50000, (B, J), generator=g, dtype=torch.int32).to(dev)
    wl[:, :hits] = words[N - hits:, :].T                                  # words the window holds
    wl_off = torch.arange(B + 1, dtype=torch.int32, device=dev) * J
    wl_out = torch.arange(B * J, dtype=torch.int32, device=dev)
    edge = -5.0 + torch.randn(B * J * beam, generator=g).to(dev)
    s = torch.zeros((B * beam, N), device=dev)
    flags = torch.zeros(1, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream().cuda_stream

    def query():
        assert lib.jlm_cache_cell_query(q.data_ptr(), H, 1, 2.0 ** 14, g0.data_ptr(), cnt.data_ptr(), slen.data_ptr(), 0, B, beam, hist.data_ptr(),
                                        count.data_ptr(), N, B, idx.data_ptr(), N, 0.3, s.data_ptr(), N, flags.data_ptr(), st) == 0

    def patch():
        assert lib.jlm_cache_cell_patch(s.data_ptr(), N, words.data_ptr(), count.data_ptr(), N, B, idx.data_ptr(), N, 0.1, cnt.data_ptr(),
                                        slen.data_ptr(), 0, B, beam, wl.data_ptr(), wl_off.data_ptr(), idx.data_ptr(), 0, wl_out.data_ptr(),
                                        edge.data_ptr(), None, B * beam, 0, None, None, flags.data_ptr(), st) == 0

    def bracket(fn):
        ms = []
        for _ in range(reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / inner)
        return ms[1:]
    tq = bracket(query)
    tp = bracket(lambda: (query(), patch()))      # (the patch overwrites s with e: every patch launch gets fresh scores)
    mq, mp = float(np.median(tq)), float(np.median(tp)) - float(np.median(tq))
    nbytes = B * N * H * 4
    return {"query_ms": round(mq, 4), "query_min": round(min(tq), 4), "query_max": round(max(tq), 4), "patch_ms": round(mp, 4),
            "query_plus_patch_ms": round(float(np.median(tp)), 4), "query_bytes": nbytes, "query_TB_per_s": round(nbytes / mq * 1e-9, 3),
            "flags": int(flags.cpu()[0])}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", default=None, help="fixture directory (default: a temporary one)")
    ap.add_argument("--steps", type=int, default=20, help="256-sentence steps per call")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--only-plain", action="store_true", help="the no_cache leg alone; one JSON line on stdout, no file")
    ap.add_argument("--repo", default=None, help="import jlm_amd from this checkout (A/B against another commit)")
    ap.add_argument("--tag", default=None, help="name of this run in its JSON line")
    ap.add_argument("--ab-file", default=None, help="JSON lines of --only-plain runs to embed under `ab_no_cache`")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "decode_cache_bench.json"))
    args = ap.parse_args(argv)
    sys.path.insert(0, os.path.abspath(args.repo) if args.repo else REPO)
    import torch
    from jlm_amd import config as jconfig, synth
    root = os.path.join(args.root or tempfile.mkdtemp(prefix="jlm_decode_cache_bench_"), "mid-vtable")
    _cfg, _lex, _rd, alphabet = synth.build_fixture(root, "mid-vtable")
    jconfig.set_root(root)
    from jlm_amd.decoder import Decoder
    dec = Decoder(1)
    B, L, beam = 256, 20, 10
    K = 4 if args.quick else args.steps
    reps = 2 if args.quick else args.repeats
    dec.max_batch = B
    sents = synth.make_sentences(B, L, seed=4242, alphabet=alphabet) * K
    V, H = dec.model.dev.V, dec.model.dev.H

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        assert len(out) == len(sents) and all(len(r) > 0 for r in out)
        return (time.perf_counter() - t0) / K * 1e3

    legs = {"no_cache": lambda: dec.decode_batch(sents, beam_width=beam)}
    out = {"bench": "decode_cache", "tag": args.tag, "device": torch.cuda.get_device_name(0), "sentences_per_step": B, "kana": L, "beam": beam,
           "steps_per_call": K, "V": V, "H": H}
    if not args.only_plain:
        from jlm_amd.cache import CacheSpec
        rng = np.random.RandomState(11)
        sizes = SIZES[:1] if args.quick else SIZES
        plain = dec.model.prime([rng.randint(2, V, size=8).tolist() for _ in sents])
        legs["context"] = lambda: dec.decode_batch(sents, beam_width=beam, context=plain)
        for N in sizes:                     # N context words a sentence: every window is full
            ctx = [rng.randint(2, V, size=N).tolist() for _ in sents]
            state = dec.model.prime(ctx, cache=CacheSpec(N, theta=0.3, lam=0.1))
            legs["cache_%d" % N] = lambda state=state: dec.decode_batch(sents, beam_width=beam, context=state)
        out["query_bytes_per_frame"] = {"cache_%d" % N: B * N * H * 4 for N in sizes}
    if not args.only_plain:
        out["kernels"] = {"cache_%d" % N: kernel_events(torch, B, beam, H, N) for N in sizes}
    for _ in range(2):                      # settle: plans, page-locked blocks and the heap of a call of this size exist afterwards
        for fn in legs.values():
            timed(fn)
    ms = {name: [] for name in legs}
    for _ in range(reps):                   # alternating
        for name, fn in legs.items():
            ms[name].append(timed(fn))
    out["legs"] = {name: _stat(v) for name, v in ms.items()}
    if args.only_plain:
        print(json.dumps(out))
        return out
    if args.ab_file and os.path.exists(args.ab_file):
        with open(args.ab_file) as f:
            out["ab_no_cache"] = [json.loads(ln) for ln in f if ln.strip().startswith("{")]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
