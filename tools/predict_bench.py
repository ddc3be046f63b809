"""Cost of converting an unfinished reading (Decoder.decode_predict_batch; csrc/jlm_tail.hip behind jlm_decode_frames): one JSON object,
printed and written to profiles/predict_bench.json.

  workload        BASELINE configs[1]: mid-vtable (LSTM h=512, D-softmax* 200/100/50, V = 50 000), 256 sentences x 20 kana, beam 10;
                  a call is `--steps` pipelined 256-sentence steps, strings -> strings (bench.py's timed region)
  legs            decode                  decode_batch(sentences)                          -- what the parent commit runs
                  decode_predict          decode_predict_batch(sentences, topN=10): the same launches + the tail launch + its read-out
                  per leg ms per 256-sentence step: median, min and max of `--repeats` calls, the legs alternating call by call so that
                  they see the same machine; before the clock two settle rounds of every leg
  tail launch     torch.ops.jlm.tail_predict alone on the pools one decoded batch left, HIP events around it: ms per launch; and the
                  frame of that decode for scale: the batch's decode time / its frames (HIP events around the frame-loop op)
  shapes          spans, extension words and candidates per sentence of the workload

    python tools/predict_bench.py [--root DIR] [--steps K] [--repeats N] [--quick] [--out FILE]
    python tools/predict_bench.py --only-plain [--repo CHECKOUT] [--tag NAME]     # the decode leg alone, one JSON line; with --repo the
                                  package is imported from another checkout (the parent commit: same launches expected)
    python tools/predict_bench.py --ab-file LINES.jsonl ...                        # embed such lines (interleaved A/B runs) in the result
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
    ap.add_argument("--only-plain", action="store_true", help="the decode leg alone; one JSON line on stdout, no file")
    ap.add_argument("--repo", default=None, help="import jlm_amd from this checkout (A/B against another commit)")
    ap.add_argument("--tag", default=None, help="name of this run in its JSON line")
    ap.add_argument("--ab-file", default=None, help="JSON lines of --only-plain runs to embed under `ab_decode`")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "predict_bench.json"))
    args = ap.parse_args(argv)
    sys.path.insert(0, os.path.abspath(args.repo) if args.repo else REPO)
    import torch
    from jlm_amd import config as jconfig, synth
    root = os.path.join(args.root or tempfile.mkdtemp(prefix="jlm_predict_bench_"), "mid-vtable")
    _cfg, _lex, _rd, alphabet = synth.build_fixture(root, "mid-vtable")
    jconfig.set_root(root)
    from jlm_amd.decoder import Decoder
    dec = Decoder(1)
    B, L, beam, topN = 256, 20, 10, 10
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
    out = {"bench": "predict", "tag": args.tag, "device": torch.cuda.get_device_name(0), "sentences_per_step": B, "kana": L, "beam": beam,
           "steps_per_call": K, "V": dec.model.dev.V}
    if not args.only_plain:
        legs["decode_predict"] = lambda: dec.decode_predict_batch(sents, topN=topN, beam_width=beam)
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
    # ---- the workload's shapes
    index = dec.model.reading_index()
    spans = [dec._tail_spans(s, index) for s in sents[:B]]
    words = [sum(hi - lo for _s, lo, hi in sp) for sp in spans]
    out["shapes"] = {"spans_per_sentence": round(float(np.mean([len(sp) for sp in spans])), 2),
                     "extension_words_per_sentence": {"mean": round(float(np.mean(words)), 1), "max": int(np.max(words))},
                     "candidates_per_sentence_at_full_beam": {"mean": round(float(np.mean(words)) * beam, 1), "max": int(np.max(words)) * beam}}
    # ---- the tail launch alone, on the pools of one decoded batch; one batch's frame loop for scale
    from jlm_amd import ops
    from jlm_amd.lattice import BatchLattice
    eng = dec._engine
    lat = BatchLattice(dec._builder, sents[:B], beam)
    off = np.zeros(B + 1, dtype=np.int32)
    np.cumsum([len(sp) for sp in spans], out=off[1:])
    flat = np.array([t for sp in spans for t in sp], dtype=np.int32).reshape(-1, 3)
    sp = (off, flat[:, 0].copy(), flat[:, 1].copy(), flat[:, 2].copy())
    dec.decode_predict_batch(sents[:B], topN=topN, beam_width=beam)          # the ids are on the device afterwards
    ev = lambda: torch.cuda.Event(enable_timing=True)
    loop_ms, tail_ms = [], []
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        e0, e1 = ev(), ev()
        e0.record()
        ticket = eng._submit(lat, "static", None, None, topN, False, predict=(sp, dec._predict_ids, dec.i2w, topN))
        e1.record()
        e1.synchronize()
        p = ticket.plan
        o = p.pr_off
        t0, t1 = ev(), ev()
        t0.record()
        ops.backend().tail_predict(dec.model.dev.decode_model(), p.obj, dec._predict_ids, p.pr_ints[o[0]:o[1]], p.pr_ints[o[1]:o[2]],
                                   p.pr_ints[o[2]:o[3]], p.pr_ints[o[3]:o[4]], topN, 0, p.pr_score, p.pr_row, p.pr_word, p.pr_nodes, p.pr_len,
                                   int(p.stride))
        t1.record()
        t1.synchronize()
        eng.collect(ticket)
        loop_ms.append(e0.elapsed_time(e1))
        tail_ms.append(t0.elapsed_time(t1))
    loop_ms, tail_ms = loop_ms[1:], tail_ms[1:]
    out["tail_launch_events"] = {"median_ms": round(float(np.median(tail_ms)), 4), "min_ms": round(float(np.min(tail_ms)), 4),
                                 "max_ms": round(float(np.max(tail_ms)), 4)}
    out["one_batch_events"] = {"note": "upload + frame loop + tail launch + read-back of ONE batch on an idle device, and per frame of it",
                               "median_ms": round(float(np.median(loop_ms)), 4), "frames": int(lat.n_frames),
                               "median_ms_per_frame": round(float(np.median(loop_ms)) / lat.n_frames, 4)}
    med = lambda name: out["legs"][name]["median_ms_per_step"]
    out["predict_minus_decode_ms_per_step"] = round(med("decode_predict") - med("decode"), 4)
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
