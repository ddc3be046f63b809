"""Cost of decoding under a memory (Decoder.decode_batch(memory=MemoryMix); csrc/jlm_memory_edge.hip, csrc/jlm_memory_topk.hip): one JSON
object, printed and written to profiles/decode_memory_bench.json.  tools/decode_cache_bench.py's method.

  workload        BASELINE configs[1]: mid-vtable (LSTM h=512, D-softmax* 200/100/50, V = 50 000), 256 sentences x 20 kana, beam 10;
                  a call is `--steps` pipelined 256-sentence steps, strings -> strings (bench.py's timed region)
  legs            no_memory               decode_batch(sentences)                      -- what the parent commit runs
                  memory_N_kK             decode_batch(sentences, memory=MemoryMix(a memory of N entries, theta 0.3, lam 0.1, k = K)):
                                          N = 10^3 / 10^4 / 10^5 at K = 64, N = 10^4 at K = 1 024; the keys are valid state rows of
                                          small random values, the words random ids
                  per leg ms per 256-sentence step: median, min and max of `--repeats` calls, the legs alternating call by call so that
                  they see the same machine; before the clock two settle rounds of every leg
  retrieval_flops 2 R N H per frame at R = 2 560 rows (x 3 f16 passes on split rows), by shape -- not a measurement
  workspace_bytes the retrieval's buffers of ONE plan (query rows, scores, words, workspace); up to four batches are in flight, each on a
                  plan of its own
  kernels         the three kernel groups ALONE, as jlm_memory_gather_rows / jlm_memory_topk / jlm_memory_cell_patch launch them for one
                  frame of the workload (256 cells x 10 slots = 2 560 live rows, H = 512 split rows, 40 list positions a cell, no
                  normaliser slices) on synthetic operands: device events around `inner` back-to-back launches, median of 7 such
                  brackets, ms per launch

    python tools/decode_memory_bench.py [--root DIR] [--steps K] [--repeats N] [--quick] [--out FILE]
    python tools/decode_memory_bench.py --only-plain [--repo CHECKOUT] [--tag NAME]   # the no_memory leg alone, one JSON line; with
                                  --repo the package is imported from another checkout (the parent commit: same launches expected)
    python tools/decode_memory_bench.py --ab-file LINES.jsonl ...                     # embed such lines (interleaved A/B runs) in the result
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((1000, 64), (10000, 64), (100000, 64), (10000, 1024))


def _stat(ms):
    return {"median_ms_per_step": round(float(np.median(ms)), 4), "min": round(float(np.min(ms)), 4), "max": round(float(np.max(ms)), 4),
            "calls": len(ms)}


def split_rows(torch, g, n, H, dev):
    """n valid split state rows of small random values (f16 hi / lo pairs viewed as float32)"""
    return (0.05 * torch.randn(n, 2 * H, generator=g)).to(torch.float16).view(torch.float32).to(dev)


def kernel_events(torch, B, beam, H, N, K, reps=7, J=40):
    """ms per launch of the three kernel groups alone at one frame's shape -> dict"""
    from jlm_amd import _lib
    from jlm_amd.memory import RetrievalBuffers
    lib, dev = _lib.lib(), torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator(device="cpu").manual_seed(N + K)
    R = B * beam
    keys, pool = split_rows(torch, g, N, H, dev), split_rows(torch, g, 2 * R, H, dev)
    key_words = torch.randint(2, 50000, (N,), generator=g, dtype=torch.int32).to(dev)
    rows = torch.randperm(2 * R, generator=g)[:R].to(torch.int32).to(dev)
    n_dev = torch.full((1,), R, dtype=torch.int32, device=dev)
    q = torch.zeros((R, H), device=dev)
    s, ret = torch.zeros((R, K), device=dev), torch.zeros((K, R), dtype=torch.int32, device=dev)
    ws = torch.zeros(max(R * (RetrievalBuffers.chunk_keys(N, R) + 2 * K), 4), device=dev)
    idx = torch.arange(B, dtype=torch.int32, device=dev)
    cnt, slen = torch.full((B,), beam, dtype=torch.int32, device=dev), torch.full((B,), 5, dtype=torch.int32, device=dev)
    base = idx * beam
    wl = torch.randint(2, 50000, (B, J), generator=g, dtype=torch.int32).to(dev)
    wl_off = torch.arange(B + 1, dtype=torch.int32, device=dev) * J
    wl_out = torch.arange(B * J, dtype=torch.int32, device=dev)
    edge = -5.0 + torch.randn(B * J * beam, generator=g).to(dev)
    flags = torch.zeros(1, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream().cuda_stream

    def gather():
        assert lib.jlm_memory_gather_rows(pool.data_ptr(), H, 2 * R, rows.data_ptr(), n_dev.data_ptr(), R, q.data_ptr(), st) == 0

    def retrieve():
        assert lib.jlm_memory_topk(keys.data_ptr(), key_words.data_ptr(), N, H, 1, 2.0 ** 14, q.data_ptr(), R, n_dev.data_ptr(), 0.3, K, s.data_ptr(),
                                   K, ret.data_ptr(), None, R, ws.data_ptr(), ws.numel() * 4, flags.data_ptr(), st) == 0

    def patch():
        assert lib.jlm_memory_cell_patch(s.data_ptr(), K, ret.data_ptr(), R, N, K, 0.1, cnt.data_ptr(), slen.data_ptr(), 0, B, beam, wl.data_ptr(),
                                         wl_off.data_ptr(), idx.data_ptr(), 0, wl_out.data_ptr(), edge.data_ptr(), None, R, 0, base.data_ptr(),
                                         None, flags.data_ptr(), st) == 0

    def bracket(fn, inner):
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
    gather()
    retrieve()                                   # the patch reads a real retrieval's lists (it rewrites edge only: every launch sees the same)
    out = {}
    for name, fn, inner in (("gather", gather, 20), ("retrieval", retrieve, 20 if N <= 10000 else 4), ("patch", patch, 20)):
        t = bracket(fn, inner)
        out[name + "_ms"] = round(float(np.median(t)), 4)
        out[name + "_min"], out[name + "_max"] = round(min(t), 4), round(max(t), 4)
    flops = 2.0 * R * N * H
    out["retrieval_flops"] = flops
    out["retrieval_TFLOP_per_s"] = round(flops / out["retrieval_ms"] * 1e-9, 2)
    out["gather_bytes"] = 2 * R * H * 4
    out["flags"] = int(flags.cpu()[0])
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", default=None, help="fixture directory (default: a temporary one)")
    ap.add_argument("--steps", type=int, default=20, help="256-sentence steps per call")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--only-plain", action="store_true", help="the no_memory leg alone; one JSON line on stdout, no file")
    ap.add_argument("--repo", default=None, help="import jlm_amd from this checkout (A/B against another commit)")
    ap.add_argument("--tag", default=None, help="name of this run in its JSON line")
    ap.add_argument("--ab-file", default=None, help="JSON lines of --only-plain runs to embed under `ab_no_memory`")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "decode_memory_bench.json"))
    args = ap.parse_args(argv)
    sys.path.insert(0, os.path.abspath(args.repo) if args.repo else REPO)
    import torch
    from jlm_amd import config as jconfig, synth
    root = os.path.join(args.root or tempfile.mkdtemp(prefix="jlm_decode_memory_bench_"), "mid-vtable")
    _cfg, _lex, _rd, alphabet = synth.build_fixture(root, "mid-vtable")
    jconfig.set_root(root)
    from jlm_amd.decoder import Decoder
    dec = Decoder(1)
    B, L, beam = 256, 20, 10
    K = 4 if args.quick else args.steps
    reps = 2 if args.quick else args.repeats
    dec.max_batch = B
    sents = synth.make_sentences(B, L, seed=4242, alphabet=alphabet) * K
    m = dec.model.dev
    V, H = m.V, m.H

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        assert len(out) == len(sents) and all(len(r) > 0 for r in out)
        return (time.perf_counter() - t0) / K * 1e3

    legs = {"no_memory": lambda: dec.decode_batch(sents, beam_width=beam)}
    out = {"bench": "decode_memory", "tag": args.tag, "device": torch.cuda.get_device_name(0), "sentences_per_step": B, "kana": L, "beam": beam,
           "steps_per_call": K, "V": V, "H": H}
    if not args.only_plain:
        from jlm_amd.engine import _MemoryBufs
        from jlm_amd.memory import Memory, MemoryMix
        assert m.split_lstm, "the workload's model keeps split state rows"
        shapes = SHAPES[:1] if args.quick else SHAPES
        g = torch.Generator(device="cpu").manual_seed(7)
        R = B * beam
        out["retrieval_flops_per_frame"], out["workspace_bytes_per_plan"], out["kernels"] = {}, {}, {}
        for N, k in shapes:
            name = "memory_%d_k%d" % (N, k)
            mem = Memory(m, split_rows(torch, g, N, H, m.device), torch.randint(2, V, (N,), generator=g, dtype=torch.int32).to(m.device))
            mx = MemoryMix(mem, theta=0.3, lam=0.1, k=k)
            legs[name] = lambda mx=mx: dec.decode_batch(sents, beam_width=beam, memory=mx)
            out["retrieval_flops_per_frame"][name] = 2.0 * R * N * H
            out["workspace_bytes_per_plan"][name] = 4 * (R * H + 2 * R * k + _MemoryBufs.workspace_floats(N, R, k))
            out["kernels"][name] = kernel_events(torch, B, beam, H, N, k)
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
            out["ab_no_memory"] = [json.loads(ln) for ln in f if ln.strip().startswith("{")]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
