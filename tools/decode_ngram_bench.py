"""Cost of decoding under an n-gram mixture (Decoder.decode_batch(ngram=NGramMix); csrc/jlm_ngram_edge.hip): one JSON object, printed
and written to profiles/decode_ngram_bench.json.  Built like tools/decode_cache_bench.py.

  workload        BASELINE configs[1]: mid-vtable (LSTM h=512, D-softmax* 200/100/50, V = 50 000), 256 sentences x 20 kana, beam 10;
                  a call is `--steps` pipelined 256-sentence steps, strings -> strings (bench.py's timed region)
  legs            no_ngram                        decode_batch(sentences)              -- what the parent commit runs (ngram = NULL)
                  ngram_o2_1e5 / o3_1e5 / o2_1e6 / o3_1e6   decode_batch(sentences, ngram=<a synthetic table of about 10^5 / 10^6
                                                  entries read at order 2 / 3>)
                  per leg ms per 256-sentence step: median, min and max of `--repeats` calls, the legs alternating call by call so that
                  they see the same machine; before the clock two settle rounds of every leg
  tables          synthetic: every unigram of the vocabulary, then random bigrams and trigrams (half each) up to the size; values random.
                  The lattice's words meet the unigrams always and the longer n-grams rarely: most look-ups walk the whole back-off.
  kernel          ngram_cell_patch_kernel ALONE, as jlm_ngram_cell_patch launches it for one frame of the workload (256 cells x 10 slots,
                  40 list positions a cell, depth-2 histories, no normaliser slices) on synthetic operands: device events around 20
                  back-to-back launches, median of 7 such brackets, ms per launch

    python tools/decode_ngram_bench.py [--root DIR] [--steps K] [--repeats N] [--quick] [--out FILE]
    python tools/decode_ngram_bench.py --only-plain [--repo CHECKOUT] [--tag NAME]   # the no_ngram leg alone, one JSON line; with --repo
                                  the package is imported from another checkout (the parent commit: same launches expected)
    python tools/decode_ngram_bench.py --ab-file LINES.jsonl ...                      # embed such lines (interleaved A/B runs) in the result
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (100000, 1000000)


def _stat(ms):
    return {"median_ms_per_step": round(float(np.median(ms)), 4), "min": round(float(np.min(ms)), 4), "max": round(float(np.max(ms)), 4),
            "calls": len(ms)}


def synthetic_table(V, n, seed):
    """an order-3 NGramTable of about n entries over V words: all unigrams, random bigrams and trigrams"""
    from jlm_amd.ngram import NGramTable
    rng = np.random.RandomState(seed)
    more = max(n - V, 0)
    w = lambda k: rng.randint(0, V, size=k).astype(np.int64) + 1
    keys = np.concatenate([np.arange(1, V + 1, dtype=np.int64), w(more // 2) | (w(more // 2) << 21),
                           w(more - more // 2) | (w(more - more // 2) << 21) | (w(more - more // 2) << 42)])
    keys = np.unique(keys)
    lp = -rng.uniform(0.1, 12.0, size=keys.size).astype(np.float32)
    bow = np.where(keys < (1 << 42), -rng.uniform(0.0, 2.0, size=keys.size), 0.0).astype(np.float32)
    return NGramTable(keys, lp, bow, 3)


def kernel_events(torch, table, order, B, beam, V, reps=7, inner=20, J=40):
    """ms per launch of the patch kernel alone at one frame's shape -> dict"""
    from jlm_amd import _lib
    lib, dev = _lib.lib(), torch.device("cuda", torch.cuda.current_device())
    arr = table.device_arrays()
    g = torch.Generator(device="cpu").manual_seed(len(table))
    keys = torch.from_numpy(arr["keys"].view(np.int64)).to(dev)
    vals = torch.from_numpy(arr["vals"]).to(dev)
    rmax = B * beam
    i32 = lambda t: t.to(torch.int32).to(dev)
    # rows 0 .. rmax - 1: an older frame (each continues a row of its own cell two frames back: bp >= 0 is all the kernel asks),
    # rows rmax .. 2 rmax - 1: the frame patched
    bp = i32(torch.cat([torch.zeros(rmax), torch.randint(0, rmax, (rmax,), generator=g)]))
    word = i32(torch.randint(2, V, (2 * rmax,), generator=g))
    score = torch.rand(2 * rmax, generator=g, dtype=torch.float64).to(dev)
    g0 = i32(rmax + torch.arange(B) * beam)
    cnt, slen = i32(torch.full((B,), beam)), i32(torch.full((B,), 5))
    root = i32(torch.tensor([[-1, 1]]).repeat(B, 1))
    idx = i32(torch.arange(B))
    wl = i32(torch.randint(2, V, (B, J), generator=g))
    wl_off, wl_out = i32(torch.arange(B + 1) * J), i32(torch.arange(B * J))
    edge = (-5.0 + torch.randn(B * J * beam, generator=g)).to(dev)
    flags = torch.zeros(1, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream().cuda_stream

    def patch():
        assert lib.jlm_ngram_cell_patch(keys.data_ptr(), vals.data_ptr(), arr["log2cap"], arr["max_probe"], order, 0.3, g0.data_ptr(),
                                        cnt.data_ptr(), slen.data_ptr(), 0, B, beam, bp.data_ptr(), word.data_ptr(), score.data_ptr(),
                                        root.data_ptr(), wl.data_ptr(), wl_off.data_ptr(), idx.data_ptr(), 0, wl_out.data_ptr(),
                                        edge.data_ptr(), None, rmax, 0, None, None, flags.data_ptr(), st) == 0

    ms = []
    for _ in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            patch()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / inner)
    ms = ms[1:]
    return {"patch_ms": round(float(np.median(ms)), 4), "min": round(min(ms), 4), "max": round(max(ms), 4), "entries": len(table),
            "log2cap": arr["log2cap"], "max_probe": arr["max_probe"], "table_MB": round((arr["keys"].nbytes + arr["vals"].nbytes) / 1e6, 1),
            "pairs": B * beam * J, "flags": int(flags.cpu()[0])}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", default=None, help="fixture directory (default: a temporary one)")
    ap.add_argument("--steps", type=int, default=20, help="256-sentence steps per call")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--only-plain", action="store_true", help="the no_ngram leg alone; one JSON line on stdout, no file")
    ap.add_argument("--repo", default=None, help="import jlm_amd from this checkout (A/B against another commit)")
    ap.add_argument("--tag", default=None, help="name of this run in its JSON line")
    ap.add_argument("--ab-file", default=None, help="JSON lines of --only-plain runs to embed under `ab_no_ngram`")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "decode_ngram_bench.json"))
    args = ap.parse_args(argv)
    sys.path.insert(0, os.path.abspath(args.repo) if args.repo else REPO)
    import torch
    from jlm_amd import config as jconfig, synth
    root = os.path.join(args.root or tempfile.mkdtemp(prefix="jlm_decode_ngram_bench_"), "mid-vtable")
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

    legs = {"no_ngram": lambda: dec.decode_batch(sents, beam_width=beam)}
    out = {"bench": "decode_ngram", "tag": args.tag, "device": torch.cuda.get_device_name(0), "sentences_per_step": B, "kana": L, "beam": beam,
           "steps_per_call": K, "V": V, "H": H}
    if not args.only_plain:
        from jlm_amd.ngram import NGramMix, NGramTable
        out["kernel"] = {}
        for n in (SIZES[:1] if args.quick else SIZES):
            table = synthetic_table(V, n, seed=n)
            for order in (2, 3):
                name = "o%d_1e%d" % (order, round(np.log10(n)))
                keep = table.keys < (1 << (21 * order))
                sub = table if order == 3 else NGramTable(table.keys[keep], table.lp[keep], table.bow[keep], order)
                mix = NGramMix(sub, 0.3)
                legs["ngram_" + name] = lambda mix=mix: dec.decode_batch(sents, beam_width=beam, ngram=mix)
                out["kernel"][name] = kernel_events(torch, mix.table, order, B, beam, V)
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
            out["ab_no_ngram"] = [json.loads(ln) for ln in f if ln.strip().startswith("{")]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
