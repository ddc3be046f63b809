"""Time of scalar k-means compression on the device (jlm_amd.compress, csrc jlm_kmeans1d): one JSON line.

  models          mid-vtable (BASELINE configs[1]'s model, V = 50 000) and mid-tied (tied softmax, V = 50 000), bit 8
  per tensor      wall seconds of kmeans_device (upload, the op, read-back of the codes), median of the repeats after one warm-up call;
                  Lloyd passes to the stop rule; HIP-event medians of the op's phases: range, histogram (the host's wait for the range
                  included), seeding (2 K + 2 launches), all Lloyd passes (the host's flag reads included), final assignment
  per model       the sum of the tensors' medians, and compress_experiment's own wall time (files included, debug text dumps off)
  Lloyd pass      on the model's largest tensor, tol = 0 and max_iter = 64: no early stop, so the event time over 64 is one pass
                  (assign + update) with the flag reads amortised; bytes = 4 n (x read once), against the 8.0 TB/s HBM peak and the
                  6.29 TB/s a float4 copy measures on this part
  scikit-learn    if it imports: KMeans(n_clusters=256, n_init=1, random_state=0) on the FIRST 1M values of that tensor on this
                  machine's CPUs -- a slice, named as one, not extrapolated

    python tools/compress_bench.py [--root DIR] [--repeats N] [--quick]
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

PHASES = ("range", "histogram", "seeding", "lloyd", "final")
HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", default=None, help="fixture directory (default: a temporary one)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args(argv)
    root = args.root or tempfile.mkdtemp(prefix="jlm_compress_bench_")
    reps = 2 if args.quick else args.repeats
    import torch
    from jlm_amd import compress as C, config as jconfig, synth, weights as W
    out = {"bench": "compress", "device": torch.cuda.get_device_name(0), "bit": 8, "repeats": reps}
    for name in ("mid-vtable", "mid-tied"):
        d = os.path.join(root, name)
        if not os.path.exists(os.path.join(d, "train", "experiments", "1", "config.json")):
            synth.build_fixture(d, name)
        jconfig.set_root(d)
        raw = W.load_weights(1)
        res = out[name] = {"tensors": {}}
        total = 0.0
        for k, v in raw.items():
            C.kmeans_device(v, 8)
            ts, ms, it = [], [], 0
            for _ in range(reps):
                t0 = time.perf_counter()
                _code, _book, info = C.kmeans_device(v, 8, timed=True)
                ts.append(time.perf_counter() - t0)
                ms.append(info["ms"])
                it = info["n_iter"]
            med = np.median(np.array(ms), axis=0)
            t = float(np.median(ts))
            total += t
            res["tensors"][k] = {"shape": list(v.shape), "n": int(v.size), "s": round(t, 5), "lloyd_passes": it,
                                 "ms": {p: round(float(x), 4) for p, x in zip(PHASES, med)}}
        res["model_s_sum_of_tensors"] = round(total, 4)
        t0 = time.perf_counter()
        C.compress_experiment(1, bit=8, debug=False)
        res["compress_experiment_s"] = round(time.perf_counter() - t0, 4)
        big = max(raw, key=lambda k: raw[k].size)
        x = torch.from_numpy(np.ascontiguousarray(raw[big], dtype=np.float32)).cuda()
        C.kmeans_device(x, 8, max_iter=64, tol=0.0)
        per = []
        for _ in range(reps):
            _c, _b, info = C.kmeans_device(x, 8, max_iter=64, tol=0.0, timed=True)
            per.append(info["ms"][3] / max(info["n_iter"], 1))
        pass_ms = float(np.median(per))
        nbytes = 4 * raw[big].size
        res["lloyd_pass"] = {"tensor": big, "n": int(raw[big].size), "passes": int(info["n_iter"]), "ms": round(pass_ms, 4),
                             "bytes": nbytes, "TB_per_s": round(nbytes / (pass_ms * 1e-3) / 1e12, 3),
                             "of_hbm_peak": round(nbytes / (pass_ms * 1e-3) / HBM_PEAK, 3),
                             "of_float4_copy": round(nbytes / (pass_ms * 1e-3) / HBM_COPY, 3)}
        try:
            from sklearn.cluster import KMeans
            sl = raw[big].reshape(-1)[:1000000].astype(np.float64).reshape(-1, 1)
            t0 = time.perf_counter()
            km = KMeans(n_clusters=256, n_init=1, random_state=0).fit(sl)
            dt = time.perf_counter() - t0
            t0 = time.perf_counter()
            code, book = C.kmeans_compress(sl.astype(np.float32).reshape(-1), 8)
            ours_t = time.perf_counter() - t0
            ours = float(((sl.reshape(-1) - np.take(book, code).astype(np.float64)) ** 2).sum())
            res["sklearn_first_1M_values"] = {"tensor": big, "s": round(dt, 3), "iterations": int(km.n_iter_),
                                              "inertia": float(km.inertia_), "ours_s": round(ours_t, 4), "ours_inertia": ours,
                                              "inertia_ratio": round(ours / float(km.inertia_), 4)}
        except ImportError:
            res["sklearn_first_1M_values"] = "scikit-learn does not import here: not measured"
        del x
        torch.cuda.empty_cache()
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
