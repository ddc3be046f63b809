"""Throughput of teacher-forced scoring on the device (LSTM_Model.score / score_streams, csrc jlm_score_frames): one JSON line.

  sentence mode   mid-vtable (BASELINE configs[1]'s model): 256 x 20 and 4 096 x 20 words per call; mid-tied: 4 096 x 20
  stream mode     mid-vtable: 2 560 streams x 20-step chunks, state carried (the reference's run_epoch layout)
  per step        event times of LSTM step / T projection / normaliser / fold at 2 560 rows (Scorer.run(timed=True))
  baselines       LSTM_Model.evaluate (one predict() per word) on ~50 sentences; the numpy oracle (oracle/jlm_oracle.py) on a few

    python tools/score_bench.py [--root DIR] [--repeats N] [--quick]

tokens/s = scored words / wall seconds of the call (host encode of the arrays, upload, launches, read-back), median of the repeats
after one warm-up call.  --quick: fewer repeats and baselines (for a profiler run).
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def _model(root, name):
    from jlm_amd import config as jconfig, synth
    d = os.path.join(root, name)
    if not os.path.exists(os.path.join(d, "train", "experiments", "1", "config.json")):
        synth.build_fixture(d, name)
    jconfig.set_root(d)
    from jlm_amd.model import LSTM_Model
    return d, LSTM_Model(experiment_id=1)


def _seqs(n, L, V, seed):
    rng = np.random.RandomState(seed)
    return [list(rng.randint(1, V, size=L)) for _ in range(n)]


def _median_time(fn, repeats):
    fn()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", default=None, help="fixture directory (default: a temporary one)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args(argv)
    root = args.root or tempfile.mkdtemp(prefix="jlm_score_bench_")
    reps = 2 if args.quick else args.repeats
    import torch
    from jlm_amd.score import Scorer
    out = {"bench": "score", "device": torch.cuda.get_device_name(0)}

    d, model = _model(root, "mid-vtable")
    m = model.dev
    V = m.V
    out["mid-vtable"] = {"normaliser": "mixed (%s)" % m.mixed_fmt if m.mixed_idx else ("split" if m.split_array is not None else "f32"),
                         "lse_fixed_ref": int(m.lse_fixed_ref)}
    for n in (256, 4096):
        seqs = _seqs(n, 20, V, seed=n)
        t = _median_time(lambda: model.score(seqs, 1), reps)
        out["mid-vtable"]["sentence_%dx20" % n] = {"tokens": n * 20, "s": round(t, 5), "tokens_per_s": round(n * 20 / t, 1)}
    # stream mode: 2 560 streams, 20-step chunks, state carried from chunk to chunk
    B, steps, n_chunks = 2560, 20, 2 if args.quick else 5
    rng = np.random.RandomState(1)
    x = rng.randint(1, V, size=(B, steps * (n_chunks + 1)))
    y = rng.randint(1, V, size=x.shape)

    def streams():
        h = c = None
        for i in range(n_chunks + 1):
            _nll, h, c = model.score_streams(x[:, i * steps:(i + 1) * steps], y[:, i * steps:(i + 1) * steps], h, c)

    t = _median_time(streams, reps)
    tok = B * steps * (n_chunks + 1)
    out["mid-vtable"]["stream_2560x20"] = {"tokens": tok, "chunks": n_chunks + 1, "s": round(t, 5), "tokens_per_s": round(tok / t, 1)}
    # per-step event times at 2 560 rows (every row live every step)
    sc = Scorer(m)
    sc.run(x[:, :steps].T, y[:, :steps].T, [B] * steps, timed=True)
    sc.run(x[:, :steps].T, y[:, :steps].T, [B] * steps, timed=True)
    st = sc.last_step_ms[1:] * 1e3                                 # (step 0 starts from the zero state)
    med = np.median(st, axis=0)
    out["mid-vtable"]["step_us_2560_rows"] = {"lstm": round(float(med[0]), 2), "t_proj": round(float(med[1]), 2),
                                              "normaliser": round(float(med[2]), 2), "fold": round(float(med[3]), 2),
                                              "total": round(float(med.sum()), 2),
                                              "fold_frac": round(float(med[3] / med.sum()), 4),
                                              "tokens_per_s_from_events": round(B / (med.sum() * 1e-6), 1)}
    # baselines: evaluate() -- one predict() per word -- and the numpy oracle
    n_eval = 10 if args.quick else 50
    ev = _seqs(n_eval, 20, V, seed=5)
    t0 = time.perf_counter()
    for s in ev:
        model.evaluate(1, s)
    t = time.perf_counter() - t0
    out["mid-vtable"]["evaluate"] = {"sentences": n_eval, "tokens": 20 * n_eval, "s": round(t, 3), "tokens_per_s": round(20 * n_eval / t, 1)}
    from oracle import jlm_oracle as orc
    lm = orc.OracleDecoder(d, 1).model
    n_orc = 2 if args.quick else 4
    t0 = time.perf_counter()
    for s in ev[:n_orc]:
        h, c = lm.zero_state(1)
        w = 1
        for tgt in s:
            _p, _y, h, c, _a, _b = lm.predict([w], h, c)
            w = tgt
    t = time.perf_counter() - t0
    out["mid-vtable"]["numpy_oracle"] = {"sentences": n_orc, "tokens": 20 * n_orc, "s": round(t, 3), "tokens_per_s": round(20 * n_orc / t, 1)}
    del model, m, sc
    torch.cuda.empty_cache()

    _d, model = _model(root, "mid-tied")
    m = model.dev
    seqs = _seqs(4096, 20, m.V, seed=7)
    t = _median_time(lambda: model.score(seqs, 1), reps)
    out["mid-tied"] = {"normaliser": "mixed (%s)" % m.mixed_fmt if m.mixed_idx else ("split" if m.split_array is not None else "f32"),
                       "sentence_4096x20": {"tokens": 4096 * 20, "s": round(t, 5), "tokens_per_s": round(4096 * 20 / t, 1)}}
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
