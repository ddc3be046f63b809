"""Cost of decoding with a left context (Decoder.decode_batch(context=), LSTM_Model.prime; csrc jlm_prime_frames, seed_context_kernel):
one JSON object, printed and written to profiles/context_bench.json.

  workload        BASELINE configs[1]: mid-vtable (LSTM h=512, D-softmax* 200/100/50, V = 50 000), 256 sentences x 20 kana, beam 10;
                  a call is `--steps` pipelined 256-sentence steps, strings -> strings (bench.py's timed region)
  legs            no_context              decode_batch(sentences)                      -- what the parent commit runs
                  fresh_8 / fresh_32      decode_batch(sentences, context=<8 | 32 random words per sentence>): prime + seed + decode
                  reused                  decode_batch(sentences, context=<a ContextState primed once, 8 words>): seed + decode
                  per leg ms per 256-sentence step: median, min and max of `--repeats` calls, the legs alternating call by call so that
                  they see the same machine; before the clock two settle rounds of every leg
  priming         LSTM_Model.prime of the call's contexts by itself, HIP events around it: ms per call and per 256 contexts
  seeding         reused - no_context (medians): the gather launch and the plans' extra rows; not measured separately

    python tools/context_bench.py [--root DIR] [--steps K] [--repeats N] [--quick] [--out FILE]
    python tools/context_bench.py --only-plain [--repo CHECKOUT] [--tag NAME]     # the no_context leg alone, one JSON line; with --repo
                                  the package is imported from another checkout (the parent commit: same launches expected)
    python tools/context_bench.py --ab-file LINES.jsonl ...                        # embed such lines (interleaved A/B runs) in the result
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _stat(ms):
    return {"median_ms_per_step": round(float(np.median(ms)), 4), "min": round(float(np.min(ms)), 4), "max": round(float(np.max(ms)), 4),
            "calls": len(ms)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", default=None, help="fixture directory (default: a temporary one)")
    ap.add_argument("--steps", type=int, default=20, help="256-sentence steps per call")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--only-plain", action="store_true", help="the no_context leg alone; one JSON line on stdout, no file")
    ap.add_argument("--repo", default=None, help="import jlm_amd from this checkout (A/B against another commit)")
    ap.add_argument("--tag", default=None, help="name of this run in its JSON line")
    ap.add_argument("--ab-file", default=None, help="JSON lines of --only-plain runs to embed under `ab_no_context`")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "context_bench.json"))
    args = ap.parse_args(argv)
    sys.path.insert(0, os.path.abspath(args.repo) if args.repo else REPO)
    import torch
    from jlm_amd import config as jconfig, synth
    root = os.path.join(args.root or tempfile.mkdtemp(prefix="jlm_context_bench_"), "mid-vtable")
    _cfg, _lex, _rd, alphabet = synth.build_fixture(root, "mid-vtable")
    jconfig.set_root(root)
    from jlm_amd.decoder import Decoder
    dec = Decoder(1)
    B, L, beam = 256, 20, 10
    K = 4 if args.quick else args.steps
    reps = 2 if args.quick else args.repeats
    dec.max_batch = B
    sents = synth.make_sentences(B, L, seed=4242, alphabet=alphabet) * K
    V = dec.model.dev.V

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        assert len(out) == len(sents) and all(len(r) > 0 for r in out)
        return (time.perf_counter() - t0) / K * 1e3

    legs = {"no_context": lambda: dec.decode_batch(sents, beam_width=beam)}
    out = {"bench": "context", "tag": args.tag, "device": torch.cuda.get_device_name(0), "sentences_per_step": B, "kana": L, "beam": beam,
           "steps_per_call": K, "V": V}
    if not args.only_plain:
        rng = np.random.RandomState(11)
        ctx = {n: [rng.randint(2, V, size=n).tolist() for _ in sents] for n in (8, 32)}
        state = dec.model.prime(ctx[8])
        legs["fresh_8"] = lambda: dec.decode_batch(sents, beam_width=beam, context=ctx[8])
        legs["fresh_32"] = lambda: dec.decode_batch(sents, beam_width=beam, context=ctx[32])
        legs["reused"] = lambda: dec.decode_batch(sents, beam_width=beam, context=state)
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
    prime = {}
    for n in (8, 32):
        ev = []
        for _ in range(reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            dec.model.prime(ctx[n])
            e1.record()
            e1.synchronize()
            ev.append(e0.elapsed_time(e1))
        ev = ev[1:]
        prime["words_%d" % n] = {"contexts": len(sents), "median_ms_per_call": round(float(np.median(ev)), 4),
                                 "median_ms_per_256_contexts": round(float(np.median(ev)) / K, 4), "min_ms_per_call": round(float(np.min(ev)), 4),
                                 "max_ms_per_call": round(float(np.max(ev)), 4)}
    out["priming_events"] = prime
    med = lambda name: out["legs"][name]["median_ms_per_step"]
    out["seeding_ms_per_step"] = {"reused_minus_no_context": round(med("reused") - med("no_context"), 4),
                                  "note": "difference of two medians: the seed_context launch, the idx upload and the plans' 256 extra rows"}
    if args.ab_file and os.path.exists(args.ab_file):
        with open(args.ab_file) as f:
            out["ab_no_context"] = [json.loads(ln) for ln in f if ln.strip().startswith("{")]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
