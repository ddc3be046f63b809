"""Cost of the per-segment candidate lists (Decoder.decode_candidates_batch; csrc/jlm_alt.hip and jlm_score_frames' launches behind
jlm_decode_frames): one JSON object, printed and written to profiles/candidates_bench.json.

  workload        BASELINE configs[1]: mid-vtable (LSTM h=512, D-softmax* 200/100/50, V = 50 000), 256 sentences x 20 kana, beam 10;
                  a call is `--steps` 256-sentence steps, strings -> strings (bench.py's timed region)
  legs            decode                  decode_batch(sentences)                          -- what the parent commit runs
                  candidates_la0 / _la1 / _all   decode_candidates_batch(sentences, lookahead=0 / 1 / None): the same launches per chunk,
                                          then the head launch and 0 / 1 / the longest suffix's score steps, chunk by chunk
                  per leg ms per 256-sentence step: median, min and max of `--repeats` calls, the legs alternating call by call so that
                  they see the same machine; before the clock two settle rounds of every leg
  rows            rows and row-steps (the sum of the rows live at every score step) per device call of each candidates leg
  head launch     torch.ops.jlm.alt_frames with no score step (lookahead 0) alone on the pools one decoded batch left, HIP events
                  around it: ms per launch

    python tools/candidates_bench.py [--root DIR] [--steps K] [--repeats N] [--quick] [--out FILE]
    python tools/candidates_bench.py --only-plain [--repo CHECKOUT] [--tag NAME]  # the decode leg alone, one JSON line; with --repo the
                                  package is imported from another checkout (the parent commit: same launches expected)
    python tools/candidates_bench.py --ab-file LINES.jsonl ...                     # embed such lines (interleaved A/B runs) in the result
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


class _Counting:
    """the op backend with the shape of every alt_frames call written down"""

    def __init__(self, inner):
        self._inner, self.calls = inner, []

    def __getattr__(self, name):
        return getattr(self._inner, name)

    def alt_frames(self, *args):
        self.calls.append((int(args[-3]), int(args[-2]), int(sum(args[21]))))          # rows, steps, row-steps
        return self._inner.alt_frames(*args)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", default=None, help="fixture directory (default: a temporary one)")
    ap.add_argument("--steps", type=int, default=20, help="256-sentence steps per call")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--only-plain", action="store_true", help="the decode leg alone; one JSON line on stdout, no file")
    ap.add_argument("--repo", default=None, help="import jlm_amd from this checkout (A/B against another commit)")
    ap.add_argument("--tag", default=None, help="name of this run in its JSON line")
    ap.add_argument("--ab-file", default=None, help="JSON lines of --only-plain runs to embed under `ab_decode`")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "candidates_bench.json"))
    args = ap.parse_args(argv)
    sys.path.insert(0, os.path.abspath(args.repo) if args.repo else REPO)
    import torch
    from jlm_amd import config as jconfig, synth
    root = os.path.join(args.root or tempfile.mkdtemp(prefix="jlm_candidates_bench_"), "mid-vtable")
    _cfg, _lex, _rd, alphabet = synth.build_fixture(root, "mid-vtable")
    jconfig.set_root(root)
    from jlm_amd.decoder import Decoder
    dec = Decoder(1)
    B, L, beam = 256, 20, 10
    K = 4 if args.quick else args.steps
    reps = 2 if args.quick else args.repeats
    dec.max_batch = B
    sents = synth.make_sentences(B, L, seed=4242, alphabet=alphabet) * K

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        assert len(out) == len(sents) and all(len(r) > 0 for r in out)
        return (time.perf_counter() - t0) / K * 1e3

    legs = {"decode": lambda: dec.decode_batch(sents, beam_width=beam)}
    out = {"bench": "candidates", "tag": args.tag, "device": torch.cuda.get_device_name(0), "sentences_per_step": B, "kana": L, "beam": beam,
           "steps_per_call": K, "V": dec.model.dev.V}
    if not args.only_plain:
        for name, la in (("candidates_la0", 0), ("candidates_la1", 1), ("candidates_all", None)):
            legs[name] = lambda la=la: dec.decode_candidates_batch(sents, beam_width=beam, lookahead=la)
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
    # ---- rows and row-steps per device call
    from jlm_amd import ops
    counting = _Counting(ops.backend())
    ops.set_backend(counting)
    try:
        out["rows"] = {}
        for name, la in (("candidates_la0", 0), ("candidates_la1", 1), ("candidates_all", None)):
            del counting.calls[:]
            dec.decode_candidates_batch(sents[:B], beam_width=beam, lookahead=la)
            out["rows"][name] = {"device_calls": len(counting.calls), "rows_per_call": [c[0] for c in counting.calls],
                                 "steps_per_call": [c[1] for c in counting.calls], "row_steps_per_call": [c[2] for c in counting.calls]}
    finally:
        ops.set_backend(counting._inner)
    # ---- the head launch alone, on the pools of one decoded batch
    from jlm_amd.lattice import BatchLattice
    eng = dec._engine
    ev = lambda: torch.cuda.Event(enable_timing=True)
    head_ms = []
    timing = _Counting(ops.backend())

    def timed_alt(*a):
        t0, t1 = ev(), ev()
        t0.record()
        r = timing._inner.alt_frames(*a)
        t1.record()
        t1.synchronize()
        head_ms.append(t0.elapsed_time(t1))
        return r
    timing.alt_frames = timed_alt
    ops.set_backend(timing)
    try:
        for _ in range(reps + 1):
            lat = BatchLattice(dec._builder, sents[:B], beam)
            ticket = eng.submit(lat, "static")
            eng.collect(ticket, keep=True)
            try:
                eng.candidates(ticket, 0, 0, 10)
            finally:
                ticket.plan.busy = False
    finally:
        ops.set_backend(timing._inner)
    head_ms = head_ms[1:]
    out["head_launch_events"] = {"note": "alt_frames with no score step: the uploads are outside the bracket, the head launch inside",
                                 "median_ms": round(float(np.median(head_ms)), 4), "min_ms": round(float(np.min(head_ms)), 4),
                                 "max_ms": round(float(np.max(head_ms)), 4)}
    med = lambda name: out["legs"][name]["median_ms_per_step"]
    out["candidates_minus_decode_ms_per_step"] = {name: round(med(name) - med("decode"), 4) for name in legs if name != "decode"}
    if args.ab_file and os.path.exists(args.ab_file):
        with open(args.ab_file) as f:
            out["ab_decode"] = [json.loads(ln) for ln in f if ln.strip().startswith("{")]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
