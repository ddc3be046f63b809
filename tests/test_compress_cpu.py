"""CPU-only: the k-means compressor's numpy restatement (jlm_amd.compress.kmeans_reference -- the arithmetic csrc/jlm_kmeans.hip
performs, which tests/test_gpu_compress.py compares byte for byte), compress_experiment's files, and the command line."""
import os
import pickle

import numpy as np
import pytest

from jlm_amd import _lib, compress, config as jconfig, synth, weights as W
from tests.compress_cases import draw as _draw


@pytest.mark.parametrize("bit", [1, 2, 3, 4, 5, 6, 7, 8])
def test_reference_shapes_order_and_nearest(bit):
    x = _draw("gauss", 30009).reshape(3, 10003)
    info = {}
    code, book = compress.kmeans_reference(x, bit, seed=3, info=info)
    K = 1 << bit
    assert code.dtype == np.uint8 and code.shape == x.shape
    assert book.dtype == np.float32 and book.shape == (K, 1)
    assert np.all(np.diff(book[:, 0]) >= 0), "codebook ascending"
    assert int(code.max()) < K and 1 <= info["n_iter"] <= 300 and not info["constant"]
    # the midpoint rule, on the grid the restatement works on: centres from the codebook (c = rint((book - mn) 2^e) recovers them
    # to within the float32 rounding of the codebook), so check in real numbers with that rounding as the slack
    b = book[:, 0].astype(np.float64)
    xf = x.astype(np.float64).reshape(-1)
    dist = np.abs(xf[:, None] - b[None, :]) if K <= 16 else None
    chosen = np.abs(xf - b[code.reshape(-1)])
    best = dist.min(axis=1) if dist is not None else np.abs(xf - b[np.clip(np.searchsorted((b[1:] + b[:-1]) / 2, xf), 0, K - 1)])
    slack = 2 * np.spacing(np.float32(np.abs(b).max())) + (float(x.max()) - float(x.min())) * 2.0 ** -34
    assert np.all(chosen <= best + slack)
    # a value strictly inside a cell has exactly the searchsorted-left code
    mids = (b[1:] + b[:-1]) / 2
    want = np.searchsorted(mids, xf, side="left")
    clear = np.abs(xf[:, None] - mids[None, :]).min(axis=1) > slack if K > 1 else np.ones(len(xf), bool)
    np.testing.assert_array_equal(code.reshape(-1)[clear], want[clear])


@pytest.mark.parametrize("name,bit", [("gauss", 8), ("t3", 4), ("uniform", 1), ("laplace", 6)])
def test_reference_is_a_lloyd_fixed_point_within_the_stop_rule(name, bit):
    """one more Lloyd pass on the returned centres moves none of them by more than the stop rule's threshold (plus the float32
    rounding of the codebook, through which the centres are read back)"""
    x = _draw(name, 50000)
    info = {}
    code, book = compress.kmeans_reference(x, bit, seed=0, info=info)
    assert info["n_iter"] < 300, "the stop rule ended it, not max_iter"
    mn, mx = float(x.min()), float(x.max())
    b = book[:, 0].astype(np.float64)
    K = 1 << bit
    cnt = np.bincount(code, minlength=K)
    mean = np.bincount(code, weights=x.astype(np.float64), minlength=K) / np.maximum(cnt, 1)
    shift = np.abs(np.where(cnt > 0, mean - b, 0.0)).max()
    assert shift <= 1e-4 * (mx - mn) + np.spacing(np.float32(np.abs(b).max())) + (mx - mn) * 2.0 ** -34, shift


def test_reference_same_seed_same_bytes_other_seed_other_picks():
    x = _draw("laplace", 40000)
    a = compress.kmeans_reference(x, 6, seed=11)
    b = compress.kmeans_reference(x.copy(), 6, seed=11)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    mn, mx = float(x.min()), float(x.max())
    e, _thr = compress.grid_params(mn, mx, 1e-4)
    hist = np.bincount((compress.quantise(x, mn, e) >> np.uint64(18)).astype(np.int64), minlength=1 << 18)
    s11 = compress.seed_reference(hist, 64, compress.TRIALS[6], 11)
    s12 = compress.seed_reference(hist, 64, compress.TRIALS[6], 12)
    assert s11 == compress.seed_reference(hist, 64, compress.TRIALS[6], 11) and s11 != s12
    assert len(set(s11)) == 64, "a bin at distance zero is never drawn"


def test_mix_is_generates_mixer():
    """splitmix64 as jlm_sample_rows documents it (include/jlm_hip.h), all 64 bits kept"""
    z = (5 + 0x9E3779B97F4A7C15 * ((3 << 32) | 2)) % 2 ** 64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) % 2 ** 64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) % 2 ** 64
    assert compress.mix(5, 3, 1) == z ^ (z >> 31)
    assert compress.TRIALS == {b: 2 + int(np.floor(np.log(2.0 ** b))) for b in range(1, 9)}


@pytest.mark.parametrize("value", [0.0, -0.0, 0.37, -1e-30, 3e38])
@pytest.mark.parametrize("bit", [1, 8])
def test_constant_tensor(value, bit):
    x = np.full((5, 7), value, np.float32)
    info = {}
    code, book = compress.kmeans_reference(x, bit, info=info)
    assert info == dict(n_iter=0, constant=True)
    assert not code.any() and book.shape == (1 << bit, 1)
    np.testing.assert_array_equal(np.take(book, code), x)


@pytest.mark.parametrize("bit,n_values", [(1, 2), (3, 8), (4, 5), (8, 256), (8, 100)])
def test_at_most_k_distinct_values_are_kept_exactly(bit, n_values):
    """multiples of 1/8 (further apart than the seeding grid): every round seeds a new value until all are centres, then repeats the
    last centre; zero inertia, the decoded tensor IS the input"""
    rng = np.random.default_rng(bit * 100 + n_values)
    vals = (np.arange(n_values) - n_values // 3) / 8.0
    x = rng.choice(vals, size=3001).astype(np.float32)
    x[:n_values] = vals
    code, book = compress.kmeans_reference(x, bit, seed=5)
    np.testing.assert_array_equal(np.take(book, code), x)
    assert np.all(np.diff(book[:, 0]) >= 0)


@pytest.mark.parametrize("n", [1, 2, 3, 5, 6, 7, 1001, 4099])
def test_small_and_ragged_sizes(n):
    x = _draw("gauss", n, seed=n)
    for bit in (1, 4, 8):
        code, book = compress.kmeans_reference(x, bit)
        assert code.shape == (n,) and book.shape == (1 << bit, 1) and np.all(np.diff(book[:, 0]) >= 0)
        if n <= (1 << bit):
            np.testing.assert_allclose(np.take(book, code), x, rtol=0, atol=(float(x.max()) - float(x.min())) * 2.0 ** -17 + 1e-9)


def test_bad_arguments():
    x = _draw("gauss", 100)
    for bit in (0, 9, -1, 32, 2.0, None):
        with pytest.raises(ValueError):
            compress.kmeans_reference(x, bit)
    for bad in (np.nan, np.inf, -np.inf):
        y = x.copy()
        y[17] = bad
        with pytest.raises(ValueError):
            compress.kmeans_reference(y, 8)
    with pytest.raises(ValueError):
        compress.kmeans_reference(np.zeros((0, 4), np.float32), 8)
    with pytest.raises(ValueError):
        compress.kmeans_reference(x, 8, max_iter=0)
    with pytest.raises(ValueError):
        compress.kmeans_reference(x, 8, seed=-1)
    with pytest.raises(ValueError):
        compress.check_args(np.broadcast_to(np.float32(0), (1 << 27) + 1), 8, 0, 300, 1e-4)


QUALITY = [(d, k) for d in ("gauss", "t3", "uniform", "bimodal", "laplace") for k in (2, 16, 256)] + [("t2", 256)]


@pytest.mark.parametrize("name,K", QUALITY)
def test_quality_against_sklearn(name, K):
    """inertia of the decoded tensor <= 1.10 x scikit-learn's KMeans(n_clusters=K, n_init=1, random_state=0) on 400 000 samples"""
    cluster = pytest.importorskip("sklearn.cluster")
    x = _draw(name, 400000)
    code, book = compress.kmeans_reference(x, {2: 1, 16: 4, 256: 8}[K], seed=0)
    xf = x.astype(np.float64)
    ours = float(((xf - np.take(book, code).astype(np.float64)) ** 2).sum())
    theirs = float(cluster.KMeans(n_clusters=K, n_init=1, random_state=0).fit(xf.reshape(-1, 1)).inertia_)
    print("%s K=%d: inertia %.6g, sklearn %.6g, ratio %.4f" % (name, K, ours, theirs, ours / theirs))
    assert ours <= 1.10 * theirs


def _patched(monkeypatch):
    def ref(weight, bit=8, *, seed=0, max_iter=300, tol=1e-4):
        return compress.kmeans_reference(weight, bit, seed, max_iter, tol, info=compress.last_info)
    monkeypatch.setattr(compress, "kmeans_compress", ref)


@pytest.mark.parametrize("name", ["small-tied", "small-vtable"])
def test_compress_experiment_writes_what_the_loaders_read(name, tmp_path, monkeypatch, capsys):
    _patched(monkeypatch)
    root = str(tmp_path)
    synth.build_fixture(root, name)
    jconfig.set_root(root)
    raw = W.load_weights(1)
    report = compress.compress_experiment(1, bit=4, seed=2)
    assert [r["name"] for r in report] == list(raw)
    for r in report:
        assert r["shape"] == raw[r["name"]].shape and r["iterations"] >= 0 and r["inertia"] >= 0 and r["seconds"] >= 0
        assert 0 <= r["rel_rms"] < 0.2, r
    assert "rel rms" in compress.format_report(report)
    d = W.weights_dir(1)
    pkl = os.path.join(d, "lstm_weights_comp_4.pkl")
    dump = os.path.join(d, "comp_4", "lstm_weights_comp_dump.pkl")
    txts = [os.path.join(d, "comp_4", "%s_%s.txt" % (k, kind)) for k in raw for kind in ("code", "codebook")]
    assert os.path.exists(pkl) and os.path.exists(dump) and all(os.path.exists(t) for t in txts)
    with open(dump, "rb") as f:
        pairs = pickle.load(f)
    want = {k: compress.kmeans_reference(v, 4, seed=2) for k, v in raw.items()}
    for k, (code, book) in pairs.items():
        assert code.dtype == np.uint8 and code.shape == raw[k].shape and book.shape == (16, 1) and book.dtype == np.float32
        assert code.tobytes() == want[k][0].tobytes() and book.tobytes() == want[k][1].tobytes()
    decoded = {k: np.take(b, c) for k, (c, b) in want.items()}

    def check_loaders(text_only=False):
        got = W.load_weights(1, 4)
        assert sorted(got) == sorted(decoded)
        for k in decoded:
            if text_only:          # np.savetxt prints the codebook with 18 digits: float32 exactly; shapes of 1-d tensors survive
                np.testing.assert_array_equal(np.asarray(got[k], np.float32).reshape(decoded[k].shape), decoded[k])
            else:
                np.testing.assert_array_equal(got[k], decoded[k])
        codes = W.load_codes(1, 4)
        assert sorted(codes) == sorted(want)
        for k, (c, b) in codes.items():
            np.testing.assert_array_equal(c.reshape(want[k][0].shape), want[k][0])
            np.testing.assert_array_equal(b, want[k][1][:, 0])

    check_loaders()                  # the decoded pickle (and the dump for load_codes)
    os.remove(pkl)
    check_loaders()                  # the dump alone
    os.remove(dump)
    check_loaders(text_only=True)    # the debug text files alone
    capsys.readouterr()


def test_compress_experiment_without_debug_and_block_list(tmp_path, monkeypatch):
    _patched(monkeypatch)
    root = str(tmp_path)
    synth.build_fixture(root, "small-tied")
    jconfig.set_root(root)
    compress.compress_experiment(1, bit=2, debug=False)
    d = W.weights_dir(1)
    assert sorted(os.listdir(os.path.join(d, "comp_2"))) == ["lstm_weights_comp_dump.pkl"]
    root2 = os.path.join(root, "ds")
    synth.build_fixture(root2, "small-dsoftmax")
    jconfig.set_root(root2)
    assert isinstance(W.load_weights(1)["LM"], list)
    with pytest.raises(ValueError):
        compress.compress_experiment(1, bit=8)
    assert not os.path.exists(os.path.join(W.weights_dir(1), "lstm_weights_comp_8.pkl"))


def test_cli_arguments(tmp_path, monkeypatch, capsys):
    a = compress.build_parser().parse_args(["-e", "7", "-c", "8"])
    assert (a.experiment, a.comp, a.root, a.seed, a.debug, a.perplexity) == ("7", 8, None, 0, True, None)
    a = compress.build_parser().parse_args(["--experiment", "3", "--comp", "4", "--root", "/x", "--seed", "9", "--no-debug",
                                            "--perplexity", "t.txt"])
    assert (a.experiment, a.comp, a.root, a.seed, a.debug, a.perplexity) == ("3", 4, "/x", 9, False, "t.txt")
    _patched(monkeypatch)
    root = str(tmp_path)
    synth.build_fixture(root, "small-tied")
    report = compress.main(["-e", "1", "-c", "3", "--root", root, "--no-debug"])
    out = capsys.readouterr().out
    assert "%d tensors" % len(report) in out and os.path.exists(os.path.join(W.weights_dir(1), "lstm_weights_comp_3.pkl"))


def test_abi_entry_and_compat_shim():
    assert "jlm_kmeans1d" in _lib.EXPORTS
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "compat", "train", "comp.py")
    spec = importlib.util.spec_from_file_location("compat_train_comp", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.kmeans_compress is compress.kmeans_compress and callable(mod.compressed_trained_weights)
