"""GPU: scalar k-means compression on the device (jlm_amd.compress.kmeans_compress / compress_experiment; csrc/jlm_kmeans.hip
jlm_kmeans1d through torch.ops.jlm.kmeans1d) against its numpy restatement, BYTE FOR BYTE: codes, codebook and the number of Lloyd
passes.  One different seeding pick changes everything after it, so equality is the only bar here; it also has to hold between two
runs and between launch shapes.  Then the files: compress_experiment on the device -> Decoder(1, comp=8) decodes as the oracle does on
the decoded weights."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
from jlm_amd import compress, config as jconfig, synth, weights as W       # noqa: E402
from oracle import jlm_oracle as orc                                       # noqa: E402
from tests.compress_cases import draw as _draw                             # noqa: E402

pytestmark = pytest.mark.gpu


def _equal(x, bit, seed=0, max_iter=300, tol=1e-4, grid=0, tag=None):
    info = {}
    want_code, want_book = compress.kmeans_reference(x, bit, seed, max_iter, tol, info=info)
    code, book, got = compress.kmeans_device(x, bit, seed, max_iter, tol, grid=grid)
    tag = (tag, bit, seed, grid)
    assert code.dtype == np.uint8 and code.shape == np.shape(x) and book.dtype == np.float32 and book.shape == (1 << bit, 1), tag
    assert (got["n_iter"], got["constant"]) == (info["n_iter"], info["constant"]), (tag, got, info)
    assert book.tobytes() == want_book.tobytes(), (tag, np.abs(book - want_book).max())
    assert code.tobytes() == want_code.tobytes(), (tag, int((code != want_code).sum()))
    return code, book, got


@pytest.mark.parametrize("bit", [1, 4, 8])
@pytest.mark.parametrize("name", ["gauss", "t3", "uniform", "bimodal", "laplace"])
def test_device_equals_restatement(name, bit):
    _equal(_draw(name, 1 << 18, seed=bit), bit, seed=bit + 1, tag=name)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 255, 1023, 1025, 65537, (1 << 20) + 3])
def test_sizes(n):
    x = _draw("gauss", n, seed=n % 1000)
    for bit in (1, 4, 8):
        _equal(x, bit, tag=n)


def test_heavy_tails_and_shapes():
    _equal(_draw("t2", 1 << 20), 8, seed=4, tag="t2")
    _equal(_draw("t3", 300 * 257).reshape(300, 257), 4, tag="2-d")
    _equal(_draw("laplace", 7 * 11 * 13).reshape(7, 11, 13), 8, tag="3-d")
    _equal(_draw("gauss", 5000) * np.float32(1e-30), 8, tag="tiny range")
    _equal(_draw("gauss", 5000) * np.float32(1e30), 8, tag="huge range")
    _equal(_draw("gauss", 5000) + np.float32(1000.0), 8, tag="offset")


def test_one_large_tensor():
    """2^25 values (BASELINE's largest tensor is 2^25.6), bit 4 and a few passes: the restatement is numpy on the host"""
    x = _draw("t3", 1 << 25)
    _code, _book, info = _equal(x, 4, seed=1, max_iter=3, tag="2^25")
    assert info["n_iter"] == 3
    code, book, info = compress.kmeans_device(x, 8, seed=1, timed=True)
    print("2^25 values, bit 8: %d passes, ms range / histogram / seeding / Lloyd / final = %s" % (info["n_iter"], info["ms"]))
    assert np.all(np.diff(book[:, 0]) >= 0) and len(np.unique(code)) > 200


@pytest.mark.parametrize("case", ["constant", "zeros", "minus-zero", "eighths-2", "eighths-100", "eighths-256", "two-values-bit8"])
def test_edge_cases(case):
    rng = np.random.default_rng(3)
    if case == "constant":
        x, bit = np.full(1001, 0.37, np.float32), 8
    elif case == "zeros":
        x, bit = np.zeros((13, 5), np.float32), 4
    elif case == "minus-zero":
        x, bit = np.full(6, -0.0, np.float32), 1
    elif case == "two-values-bit8":
        x, bit = rng.choice(np.array([-1.5, 2.25], np.float32), size=4099), 8
    else:
        k = int(case.split("-")[1])
        vals = ((np.arange(k) - k // 3) / 8.0).astype(np.float32)
        x = rng.choice(vals, size=50001)
        x[:k] = vals
        bit = {2: 1, 100: 8, 256: 8}[k]
    code, book, _info = _equal(x, bit, seed=5, tag=case)
    np.testing.assert_array_equal(np.take(book, code), x)          # zero inertia: the decoded tensor is the input


def test_bad_input_raises_before_or_on_the_device():
    x = _draw("gauss", 4096)
    for bit in (0, 9):
        with pytest.raises(ValueError):
            compress.kmeans_compress(x, bit)
    for bad, at in ((np.nan, 0), (np.inf, 4095), (-np.inf, 1234)):
        y = x.copy()
        y[at] = bad
        with pytest.raises(ValueError):
            compress.kmeans_compress(y, 8)
    with pytest.raises(ValueError):
        compress.kmeans_compress(np.zeros(0, np.float32), 8)
    code, book = compress.kmeans_compress(x, 3, seed=2)             # the public name, keyword-only options
    want = compress.kmeans_reference(x, 3, seed=2)
    assert code.tobytes() == want[0].tobytes() and book.tobytes() == want[1].tobytes() and compress.last_info["n_iter"] >= 1


def test_two_runs_and_other_grids_give_the_same_bytes():
    x = _draw("laplace", (1 << 19) + 1)
    base = compress.kmeans_device(x, 8, seed=9)
    for grid in (0, 1, 7, 64, 1000):
        code, book, info = compress.kmeans_device(x, 8, seed=9, grid=grid)
        assert code.tobytes() == base[0].tobytes() and book.tobytes() == base[1].tobytes() and info["n_iter"] == base[2]["n_iter"], grid
    on_device = compress.kmeans_device(torch.from_numpy(x).cuda(), 8, seed=9)
    assert on_device[0].tobytes() == base[0].tobytes()
    other = compress.kmeans_device(x, 8, seed=10)
    assert other[1].tobytes() != base[1].tobytes()


def _same(got, want, tag):
    """the decode's score bar (tests/test_gpu_edge_cases.py)"""
    assert len(got) == len(want), tag
    assert got[0][1] == want[0][1], (tag, got[0], want[0])
    np.testing.assert_allclose([s for s, _ in got], [s for s, _ in want], rtol=2e-6, atol=2e-5, err_msg=str(tag))


@pytest.mark.parametrize("mode", ["tied", "vtable", "untied"])
def test_compress_experiment_then_decode(mode, tmp_path, capsys):
    """the sizes of test_kmeans_compressed_model_on_device, but the codebooks are k-means': resident uint8 codes, panels bit-equal to
    np.take(codebook, code), and the decode of the oracle on weights.load_weights(1, 8)"""
    root = str(tmp_path)
    cfg = synth.make_config(3000, 64, 32, mode, segs=[(32, 0, 700), (16, 700, 1800), (8, 1800, None)])
    synth.write_lexicon(root, 3000, alphabet=10)
    synth.write_experiment(root, 1, cfg, scale=0.3)
    jconfig.set_root(root)
    report = compress.compress_experiment(1, bit=8, seed=1)
    print(compress.format_report(report))
    raw = W.load_weights(1)
    assert [r["name"] for r in report] == list(raw) and all(r["iterations"] >= 0 and r["rel_rms"] < 0.05 for r in report)
    pairs = W.load_codes(1, 8)
    decoded = W.load_weights(1, 8)
    assert sorted(pairs) == sorted(raw)
    for k, (code, book) in pairs.items():
        np.testing.assert_array_equal(np.take(book, code).reshape(raw[k].shape), decoded[k])
    from jlm_amd.decoder import Decoder
    d = Decoder(1, comp=8)
    m = d.model.dev
    assert len(m.seg_codes) == m.n_segs and all(c.dtype == torch.uint8 and c.is_cuda for c, _b in m.seg_codes.values())
    names = {"tied": ["LM"], "untied": ["UM"], "vtable": ["LM0", "LM1", "LM2"]}[mode]
    for i, nm in enumerate(names):
        want = decoded[nm].T if mode == "untied" else decoded[nm]
        np.testing.assert_array_equal(m.seg_B[i].cpu().numpy()[:, :want.shape[1]], want.astype(np.float32))
    o = orc.OracleDecoder(root, 1)
    o.model = orc.OracleLM(o.config, decoded)
    sents = synth.make_ragged_sentences(10, 2, 14, seed=4, alphabet=10)
    for s, g in zip(sents, d.decode_batch(sents, beam_width=6)):
        _same(g, o.decode(s, beam_width=6), (mode, s))


def test_perplexity_of_the_compressed_model(tmp_path, capsys):
    """mid-vtable: score() perplexity of the 8-bit model against the uncompressed one.  Both finite; the ratio is PRINTED, not
    asserted: synthetic weights say nothing about what a trained model loses."""
    root = str(tmp_path)
    synth.build_fixture(root, "mid-vtable")
    jconfig.set_root(root)
    report = compress.compress_experiment(1, bit=8, debug=False)
    from jlm_amd.model import LSTM_Model
    rng = np.random.RandomState(5)
    seqs = [list(rng.randint(1, 50000, size=L)) for L in rng.randint(5, 30, size=400)]
    n_tok = sum(len(s) for s in seqs)
    pp = []
    for comp in (0, 8):
        model = LSTM_Model(experiment_id=1, comp=comp)
        nll = model.score(seqs, 1, per_token=False)
        pp.append(float(np.exp(np.sum(nll) / n_tok)))
    with capsys.disabled():
        print("\n" + compress.format_report(report))
        print("mid-vtable perplexity: uncompressed %.4f, comp_8 %.4f, ratio %.5f" % (pp[0], pp[1], pp[1] / pp[0]))
    assert np.isfinite(pp[0]) and np.isfinite(pp[1]) and pp[0] > 1 and pp[1] > 1


def test_command_line_with_perplexity(tmp_path, capsys):
    """python -m jlm_amd.compress -e 1 -c 8 --perplexity FILE: the report, then jlm_amd.perplexity on both models and their ratio"""
    import os
    root = str(tmp_path)
    cfg, lexicon, _rd, _alphabet = synth.build_fixture(root, "small-tied")
    synth.write_test_corpus(root, lexicon, cfg["vocab_size"], 600, words_per_sentence=6, seed=13, oov_every=4)   # > 64 streams x 20 steps
    report = compress.main(["-e", "1", "-c", "8", "--root", root, "--seed", "3", "--perplexity", os.path.join(root, "data", "test.txt")])
    out = capsys.readouterr().out
    assert "%d tensors" % len(report) in out and all(r["iterations"] is not None for r in report)
    line = [l for l in out.splitlines() if l.startswith("perplexity: uncompressed")]
    assert len(line) == 1 and "comp_8" in line[0], out
    base, comp, ratio = (float(line[0].split()[i]) for i in (2, 4, 6))
    assert np.isfinite(base) and np.isfinite(comp) and abs(ratio - comp / base) < 1e-4
    with capsys.disabled():
        print("\n" + line[0])
    assert os.path.exists(os.path.join(W.weights_dir(1), "comp_8", "LM_codebook.txt"))
