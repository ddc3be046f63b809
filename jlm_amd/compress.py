"""Scalar k-means compression of a model's weights on the device: ``kmeans_compress``, ``compress_experiment`` and
``python -m jlm_amd.compress``.

The reference's producer of the ``(code uint8, codebook)`` files is train/comp.py: per tensor, scikit-learn ``KMeans(2**bit)`` over the
flattened weights -- "about 1 hour" for one (50k, 512) embedding by its own docstring, and it no longer runs (``n_jobs`` is gone from
scikit-learn).  Here one tensor is ONE op (``torch.ops.jlm.kmeans1d``, csrc/jlm_kmeans.hip ``jlm_kmeans1d``): greedy k-means++ seeding
(scikit-learn's: ``2 + floor(ln K)`` trials per centre), then Lloyd's iteration, ``n_init = 1``.  The files written are the ones
``jlm_amd.weights.load_weights`` / ``load_codes`` read.

Arithmetic (pinned by tests/test_compress_cpu.py and tests/test_gpu_compress.py).  Every accumulation is an
integer sum, so the bytes that come out do not depend on the launch shape or on the order anything is added in, and
:func:`kmeans_reference` restates them exactly in numpy:
  - ``mn = min x``, ``mx = max x``; ``e`` such that ``2^35 <= (mx - mn) 2^e < 2^36``; ``q = min(rint((x - mn) 2^e), 2^36 - 1)`` in f64;
  - seeding runs on the histogram of ``v = q >> 18`` (2^18 bins): centre 0 is the bin of a uniformly drawn point; round r draws its
    trials with probability ~ count * D^2 -- target ``floor(u * total)``, ``u = splitmix64(seed, r, t) / 2^64``, the first bin whose
    inclusive prefix exceeds it -- and keeps the trial that leaves the smallest total, the lowest trial on a tie; a bin at distance
    zero is never drawn, and once the total is zero a round repeats the previous centre;
  - a seeded bin v starts Lloyd at ``(v << 18) + 2^17``.  Centres stay sorted ascending; a value belongs to the number of midpoints
    strictly below it (``2 q > c_j + c_(j+1)``: a value on a midpoint goes to the lower centre); a centre moves to the rounded integer
    mean ``(sum + count // 2) // count`` of its values, an empty centre stays; the iteration stops after the pass whose largest shift
    is ``<= floor(tol (mx - mn) 2^e)`` or after ``max_iter`` passes;
  - codes are the assignment against the final centres; ``codebook[j] = float32(mn + c_j 2^-e)``, ASCENDING (scikit-learn's order is
    arbitrary; ascending is this package's).  A constant tensor: codebook all ``mn``, codes 0.  Ascending is how k-means LEAVES a
    codebook, not something a reader may rely on: ``jlm_amd.finetune`` retrains the entries and they need not stay in order.  Every
    reader decodes with ``take(codebook, code)``.

There is no CPU fallback: ``kmeans_compress`` needs the GPU, like the rest of the package.
"""
import argparse
import math
import os
import pickle
import time

import numpy as np

from . import config as _config
from . import ops as _ops
from . import weights as _weights

last_info = {}                       # the last kmeans_compress call's n_iter / constant (compress_experiment's report reads it)
MAX_N = 1 << 27                      # JLM_KMEANS_MAX_N: every integer total fits 64 bits
SCRATCH_BYTES = (2 << 20) + 16384 + 65536    # JLM_KMEANS_SCRATCH_BYTES
GRID_BITS = 36                       # the Lloyd grid: range / 2^36 < step <= range / 2^35
SEED_SHIFT = 18                      # the seeding grid: q >> 18, 2^18 bins
TRIALS = {1: 2, 2: 3, 3: 4, 4: 4, 5: 5, 6: 6, 7: 6, 8: 7}      # 2 + floor(ln 2^bit)
_M64 = (1 << 64) - 1


def check_args(weight, bit, seed, max_iter, tol):
    """ValueError for anything the kernels cannot take, before any launch.  -> the tensor's shape"""
    is_int = lambda v: isinstance(v, (int, np.integer)) and not isinstance(v, bool)
    if not is_int(bit) or not 1 <= bit <= 8:
        raise ValueError("bit must be an integer in [1, 8]: codes wider than a byte cannot be loaded (got %r)" % (bit,))
    if not is_int(seed) or not 0 <= seed < 1 << 63:
        raise ValueError("seed must be an integer in [0, 2^63) (got %r)" % (seed,))
    if not is_int(max_iter) or max_iter < 1:
        raise ValueError("max_iter must be an integer >= 1 (got %r)" % (max_iter,))
    if not isinstance(tol, (int, float, np.floating, np.integer)) or not 0 <= float(tol) <= 1:
        raise ValueError("tol must be a number in [0, 1], a fraction of max - min (got %r)" % (tol,))
    shape = tuple(weight.shape)
    n = int(np.prod(shape, dtype=np.int64)) if shape else 1
    if n < 1:
        raise ValueError("cannot compress an empty tensor")
    if n > MAX_N:
        raise ValueError("a tensor of %d values is above the %d the 64-bit integer sums are sized for" % (n, MAX_N))
    return shape


def mix(seed, centre, trial):
    """splitmix64 of (seed, centre, trial), all 64 bits: generate's mixer (sample_rows_kernel) of (centre << 32) | (trial + 1)."""
    z = (seed + 0x9E3779B97F4A7C15 * ((centre << 32) | (trial + 1))) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def grid_params(mn, mx, tol):
    """-> (e, thr): the Lloyd grid's exponent and the stop rule's threshold in grid steps."""
    rng = float(mx) - float(mn)
    e = GRID_BITS - math.frexp(rng)[1]
    return e, min(int(math.floor(float(tol) * math.ldexp(rng, e))), 1 << 63)


def quantise(x, mn, e):
    """x float32 [n] -> q uint64 [n] on the Lloyd grid."""
    q = np.rint(np.ldexp(x.astype(np.float64) - np.float64(mn), e))
    return np.minimum(q, float((1 << GRID_BITS) - 1)).astype(np.uint64)


# ------------------------------------------------------------------------------------------------- numpy restatement (the tests')
def seed_reference(hist, K, trials, seed):
    """km_seed_kernel restated.  hist: int64 counts of the 2^18 seeding bins -> the K seeded bins in round order (list of int)."""
    h = hist.astype(np.uint64)
    v = np.arange(len(h), dtype=np.int64)
    centres = []
    w = h.copy()                                         # round 0 draws a point: weight = count
    d = None
    for r in range(K):
        L = trials if r else 1
        total = int(w.sum(dtype=np.uint64))
        if total == 0:
            cands = [centres[-1]] * L
        else:
            cum = np.cumsum(w, dtype=np.uint64)
            cands = [int(np.searchsorted(cum, np.uint64((mix(seed, r, t) * total) >> 64), side="right")) for t in range(L)]
        best = None
        for c in cands:
            dc = np.abs(v - c).astype(np.uint64)
            nd = dc if d is None else np.minimum(d, dc)
            wc = h * (nd * nd)
            s = int(wc.sum(dtype=np.uint64))
            if best is None or s < best[0]:
                best = (s, c, nd, wc)
        _s, c, d, w = best
        centres.append(c)
    return centres


def kmeans_reference(weight, bit=8, seed=0, max_iter=300, tol=1e-4, info=None):
    """The kernels' arithmetic restated in numpy (module docstring): -> (code uint8 of weight's shape, codebook float32 [2**bit, 1]).
    ``info`` (a dict, optional) receives ``n_iter`` (Lloyd passes run) and ``constant``."""
    weight = np.asarray(weight)
    shape = check_args(weight, bit, seed, max_iter, tol)
    x = np.ascontiguousarray(weight, dtype=np.float32).reshape(-1)
    if not np.isfinite(x).all():
        raise ValueError("cannot compress a tensor that holds NaN or infinity")
    K = 1 << bit
    mn, mx = float(x.min()), float(x.max())
    if info is not None:
        info.update(n_iter=0, constant=mx == mn)
    if mx == mn:
        return np.zeros(shape, np.uint8), np.full((K, 1), np.float32(mn) + np.float32(0.0), dtype=np.float32)
    e, thr = grid_params(mn, mx, tol)
    q = quantise(x, mn, e)
    hist = np.bincount((q >> np.uint64(SEED_SHIFT)).astype(np.int64), minlength=1 << SEED_SHIFT)
    c = np.array(sorted(seed_reference(hist, K, TRIALS[bit], int(seed))), dtype=np.uint64)
    c = (c << np.uint64(SEED_SHIFT)) + np.uint64(1 << (SEED_SHIFT - 1))
    q2 = q << np.uint64(1)
    qi = q.astype(np.int64)
    n_iter = 0
    for _ in range(max_iter):
        a = np.searchsorted(c[:-1] + c[1:], q2, side="left")
        cnt = np.bincount(a, minlength=K).astype(np.uint64)
        # per-centre sums < 2^63: exact in Python integers whatever numpy's reduction does
        ssum = _exact_bin_sums(a, qi, K)
        new = c.copy()
        nz = cnt > 0
        new[nz] = (ssum[nz] + cnt[nz] // np.uint64(2)) // cnt[nz]
        shift = int(np.max(np.maximum(new, c) - np.minimum(new, c)))
        c = new
        n_iter += 1
        if shift <= thr:
            break
    code = np.searchsorted(c[:-1] + c[1:], q2, side="left").astype(np.uint8).reshape(shape)
    book = (np.float64(mn) + np.ldexp(c.astype(np.float64), -e)).astype(np.float32).reshape(K, 1)
    if info is not None:
        info["n_iter"] = n_iter
    return code, book


def _exact_bin_sums(a, qi, K):
    """sum of int64 qi per bin a, exactly, as uint64 [K]: the low and high 18 bits summed apart (float64 bincount is exact below 2^53:
    n <= 2^27 values below 2^18 each)."""
    lo = np.bincount(a, weights=(qi & 0x3FFFF).astype(np.float64), minlength=K)
    hi = np.bincount(a, weights=(qi >> 18).astype(np.float64), minlength=K)
    return (hi.astype(np.uint64) << np.uint64(18)) + lo.astype(np.uint64)


# ------------------------------------------------------------------------------------------------- the device
def kmeans_device(weight, bit=8, seed=0, max_iter=300, tol=1e-4, grid=0, timed=False):
    """One tensor through ``torch.ops.jlm.kmeans1d``.  weight: numpy array or torch tensor (a tensor on the GPU is used in place).
    grid: workgroups of the streaming passes (0: four per compute unit; the bytes do not depend on it).
    -> (code uint8 numpy, codebook float32 [2**bit, 1] numpy, info dict: n_iter, constant, and with ``timed`` ms = [range, histogram,
    seeding, Lloyd passes, final assignment])"""
    import torch
    from . import _lib
    shape = check_args(weight, bit, seed, max_iter, tol)
    dev = _lib.require_gpu()
    backend = _ops.backend()
    if isinstance(weight, torch.Tensor):
        x = weight.detach().to(device=dev, dtype=torch.float32).contiguous().reshape(-1)
    else:
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(weight), dtype=np.float32).reshape(-1)).to(dev)
    K = 1 << bit
    with torch.cuda.device(dev):
        code = torch.empty(x.numel(), device=dev, dtype=torch.uint8)
        book = torch.empty(K, device=dev, dtype=torch.float32)
        scratch = torch.empty(SCRATCH_BYTES, device=dev, dtype=torch.uint8)
        out = backend.kmeans1d(x, int(bit), int(seed), int(max_iter), float(tol), code, book, scratch, int(grid), bool(timed))
    out = [float(v) for v in out]
    if out[2]:
        raise ValueError("cannot compress a tensor that holds NaN or infinity")
    info = dict(n_iter=int(out[0]), constant=bool(out[1]))
    if timed:
        info["ms"] = out[4:9]
    return code.cpu().numpy().reshape(shape), book.cpu().numpy().reshape(K, 1), info


def kmeans_compress(weight, bit=8, *, seed=0, max_iter=300, tol=1e-4):
    """train/comp.py:20 ``kmeans_compress(weight, bit=8)`` on the device: -> (code uint8 with weight's shape, codebook float32
    [2**bit, 1], ascending).  The same weight, bit and seed give the same bytes on every run, and the bytes of
    :func:`kmeans_reference`.  ``tol`` is a fraction of ``max - min``.  ValueError: bit outside [1, 8], NaN / infinity, an empty
    tensor or one above 2^27 values."""
    code, book, info = kmeans_device(weight, bit, seed, max_iter, tol)
    last_info.clear()
    last_info.update(info)
    return code, book


def compress_experiment(experiment_id, bit=8, debug=True, seed=0, max_iter=300, tol=1e-4):
    """What train/comp.py:50-80 ``compressed_trained_weights`` does: reads weights/lstm_weights.pkl of the experiment, compresses
    every tensor and writes weights/lstm_weights_comp_{bit}.pkl (decoded floats), weights/comp_{bit}/lstm_weights_comp_dump.pkl
    (name -> (code, codebook)) and, with ``debug``, {name}_code.txt / {name}_codebook.txt beside the dump.
    -> list of per-tensor reports (dicts: name, shape, iterations, inertia, rel_rms, seconds)."""
    wdir = _weights.weights_dir(experiment_id)
    with open(os.path.join(wdir, "lstm_weights.pkl"), "rb") as f:
        weights = pickle.load(f)
    for k, v in weights.items():
        if isinstance(v, list):
            raise ValueError("tensor %r is a D_softmax block list: train/comp.py cannot compress it either" % (k,))
    decoded, dump, report = {}, {}, []
    for k, v in weights.items():
        v = np.asarray(v)
        last_info.clear()
        t0 = time.time()
        code, book = kmeans_compress(v, bit, seed=seed, max_iter=max_iter, tol=tol)
        dt = time.time() - t0
        dump[k] = (code, book)
        decoded[k] = _weights.decode_codebook(code, book)
        err = decoded[k].astype(np.float64) - v.astype(np.float64)
        inertia = float((err * err).sum())
        power = float((v.astype(np.float64) ** 2).sum())
        report.append(dict(name=k, shape=tuple(v.shape), iterations=last_info.get("n_iter"), inertia=inertia,
                           rel_rms=math.sqrt(inertia / power) if power > 0 else 0.0, seconds=dt))
    write_compressed(experiment_id, bit, dump, debug)
    return report


def write_compressed(experiment_id, bit, dump, debug):
    """The files of a compressed experiment from ``dump`` (name -> (code, codebook [2^bit, 1])): weights/lstm_weights_comp_{bit}.pkl
    (``take(codebook, code)`` per tensor), weights/comp_{bit}/lstm_weights_comp_dump.pkl and, with ``debug``, the text dumps beside
    it.  ``compress_experiment`` and ``jlm_amd.finetune`` both write through here."""
    wdir = _weights.weights_dir(experiment_id)
    cdir = os.path.join(wdir, "comp_{}".format(bit))
    os.makedirs(cdir, exist_ok=True)
    decoded = {k: _weights.decode_codebook(code, book) for k, (code, book) in dump.items()}
    if debug:
        for k, (code, book) in dump.items():
            np.savetxt(os.path.join(cdir, "{}_code.txt".format(k)), np.asarray(code).astype(int), fmt="%i")
            np.savetxt(os.path.join(cdir, "{}_codebook.txt".format(k)), book)
    with open(os.path.join(wdir, "lstm_weights_comp_{}.pkl".format(bit)), "wb") as f:
        pickle.dump(decoded, f)
    with open(os.path.join(cdir, "lstm_weights_comp_dump.pkl"), "wb") as f:
        pickle.dump(dump, f)


def format_report(report):
    lines = ["%-6s %-16s %5s %14s %10s %9s" % ("tensor", "shape", "iter", "inertia", "rel rms", "seconds")]
    for r in report:
        lines.append("%-6s %-16s %5s %14.6g %10.3e %9.3f" % (r["name"], "x".join(str(s) for s in r["shape"]) or "scalar",
                                                            "-" if r["iterations"] is None else r["iterations"], r["inertia"],
                                                            r["rel_rms"], r["seconds"]))
    lines.append("%d tensors, %.3f s" % (len(report), sum(r["seconds"] for r in report)))
    return "\n".join(lines)


def build_parser():
    ap = argparse.ArgumentParser(description="Compress an experiment's weights by scalar k-means on the device "
                                             "(reference train/comp.py)")
    ap.add_argument("--experiment", "-e", dest="experiment", default="10", help="which experiment dump to use (train/comp.py's default: 10)")
    ap.add_argument("--comp", "-c", dest="comp", type=int, default=1, help="compress bit (1 .. 8)")
    ap.add_argument("--root", default=None, help="artifact root (default: jlm_amd.config's)")
    ap.add_argument("--seed", type=int, default=0, help="seed of the k-means++ draws")
    ap.add_argument("--no-debug", dest="debug", action="store_false", help="do not write the {name}_code.txt / {name}_codebook.txt dumps")
    ap.add_argument("--perplexity", default=None, metavar="TOKENS_FILE",
                    help="also print the perplexity of the uncompressed and the compressed model on this corpus, and their ratio")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.root:
        _config.set_root(args.root)
    report = compress_experiment(args.experiment, args.comp, debug=args.debug, seed=args.seed)
    print(format_report(report))
    if args.perplexity:
        from . import perplexity as _ppl
        common = ["-e", str(args.experiment), "--file", args.perplexity] + (["--root", args.root] if args.root else [])
        base = _ppl.main(common)
        comp = _ppl.main(common + ["--comp", str(args.comp)])
        print("perplexity: uncompressed {:.4f}  comp_{} {:.4f}  ratio {:.5f}".format(base, args.comp, comp, comp / base))
    return report


if __name__ == "__main__":
    main()
