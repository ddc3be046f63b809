"""GPU: fine-tuning the codebooks of a compressed model on the device (jlm_amd.finetune.CodebookDeviceStepper over
torch.ops.jlm.train_expand_codes / train_codebook_grad, csrc/jlm_train.hip) against the numpy float64 restatement
(CodebookReferenceStepper): the two kernels as launched, one step's codebook gradients, twenty steps, reproducibility, and the driver
on the Markov corpus with the fine-tuned experiment scored and decoded from its resident codes.

The kernel bars: expansion is a copy (bit-equal); a codebook gradient is one f32 rounding of an f64 sum of n_j terms (2^-24 |exact| +
n_j 2^-52 sum|g|).  The step, twenty-step and end-to-end bars are those of tests/test_gpu_train.py."""
import os
import pickle
import shutil
import tempfile

import numpy as np
import pytest

torch = pytest.importorskip("torch")
from jlm_amd import compress, config as jconfig, finetune as F, ops as jops, synth, train as T, weights as W      # noqa: E402
from tests import train_cases as tc                                                                              # noqa: E402

pytestmark = pytest.mark.gpu
CH = F.CODEBOOK_CHUNK


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


# ---- 7. expansion
@pytest.mark.parametrize("n", [4, 260, 65540])
@pytest.mark.parametrize("K", [2, 256])
def test_expand_codes(n, K):
    rng = np.random.RandomState(n + K)
    n_book = 3 * K
    book = rng.normal(size=n_book).astype(np.float32)
    gid = rng.randint(0, n_book, n).astype(np.int32)
    gid[rng.rand(n) < 0.2] = -1                                   # padding, sprinkled in
    gid[n - 1] = -1
    gid[0] = n_book - 1
    w = torch.full((n + 4,), 7.0, device="cuda")
    jops.backend().train_expand_codes(_dev(book), _dev(gid), w, n)
    got = w.cpu().numpy()
    want = np.where(gid >= 0, np.take(book, np.maximum(gid, 0)), np.float32(0.0))
    assert got[:n].tobytes() == want.astype(np.float32).tobytes()
    assert np.all(got[n:] == 7.0)                                 # nothing past n is written


# ---- 8. the codebook gradient
def _grad_case(sizes, seed):
    """groups of the given sizes scattered over a flat buffer with padding -> (g, gid, order, chunks)"""
    rng = np.random.RandomState(seed)
    K = len(sizes)
    code = rng.permutation(np.repeat(np.arange(K), sizes)).astype(np.uint8)
    n = len(code)
    n_flat = (n + 3) // 4 * 4 + 4
    gid, order, chunks = F.build_groups([("x", None, (n,), 0, n)], ["x"], {"x": code}, K, n_flat)
    g = (rng.normal(size=n_flat) * 10.0 ** rng.uniform(-6, 0, n_flat)).astype(np.float32)      # magnitudes over six decades: order shows
    return g, gid, order, chunks


@pytest.mark.parametrize("case", ["sizes", "one code"])
def test_codebook_grad(case):
    sizes = [0, 1, 63, 64, 65, CH, CH + 1, 3 * CH + 17, 0] if case == "sizes" else [0, 70000]
    g, gid, order, chunks = _grad_case(sizes, 11)
    K = len(sizes)
    assert np.array_equal(np.bincount(gid[gid >= 0], minlength=K), sizes) and chunks[:, 2].max() <= CH
    O = jops.backend()
    gd, od, cd = _dev(g), _dev(order), _dev(chunks.reshape(-1))
    outs = []
    for fill in (float("nan"), 3.0):                              # garbage in both output buffers
        partial = torch.full((len(chunks),), fill, device="cuda", dtype=torch.float64)
        gbook = torch.full((K + 3,), fill, device="cuda")
        O.train_codebook_grad(gd, od, cd, len(chunks), K, partial, gbook)
        outs.append(gbook.cpu().numpy())
    assert outs[0][:K].tobytes() == outs[1][:K].tobytes()         # the same bits, launch after launch
    assert np.isnan(outs[0][K:]).all()                            # nothing past n_groups is written
    got = outs[0][:K].astype(np.float64)
    coded = gid >= 0
    exact = np.bincount(gid[coded], weights=g[coded].astype(np.float64), minlength=K)
    mag = np.bincount(gid[coded], weights=np.abs(g[coded]).astype(np.float64), minlength=K)
    bound = 2.0 ** -24 * np.abs(exact) + np.array(sizes) * 2.0 ** -52 * mag
    print("codebook gradient: |got - exact| / bound per group:", ["%.2f" % (abs(a - b) / c) if c else "-" for a, b, c in zip(got, exact, bound)])
    assert np.all(np.abs(got - exact) <= bound)
    for j, s in enumerate(sizes):
        if s == 0:
            assert outs[0][j] == 0.0 and outs[1][j] == 0.0


def test_codebook_grad_without_chunks():
    """every group empty: the second launch alone, zeros over garbage"""
    gbook = torch.full((5,), float("nan"), device="cuda")
    empty = torch.zeros(0, device="cuda", dtype=torch.int32)
    jops.backend().train_codebook_grad(torch.ones(8, device="cuda"), empty, empty, 0, 5, torch.zeros(1, device="cuda", dtype=torch.float64), gbook)
    assert np.array_equal(gbook.cpu().numpy(), np.zeros(5, dtype=np.float32))


# ---- 9. one step
_models = {}


def _model(mode, bit):
    """(cfg, codes, books): Glorot weights quantised per tensor (computed once per case)"""
    if (mode, bit) not in _models:
        cfg = synth.make_config(600, 64, 32, mode, [(32, 0, 150), (16, 150, 360), (8, 360, None)], True)
        pairs = {k: tc.grid_quantise(v, 1 << bit) for k, v in T.init_weights(cfg, None, 101).items()}
        _models[(mode, bit)] = (cfg, {k: c for k, (c, _b) in pairs.items()}, {k: b for k, (_c, b) in pairs.items()})
    return _models[(mode, bit)]


def _batch(V, B, Tn, seed):
    rng = np.random.RandomState(seed)
    return rng.randint(0, V, (B, Tn)), rng.randint(0, V, (B, Tn))


@pytest.mark.parametrize("mode,bit,B,Tn", [("tied", 3, 32, 10), ("tied", 8, 32, 10), ("vtable", 3, 32, 10), ("vtable", 8, 32, 10),
                                           ("vtable", 3, 13, 7)])
def test_one_step(mode, bit, B, Tn):
    cfg, codes, books = _model(mode, bit)
    kw = dict(lr=1e-3, dropout=0.9, norm_weight=0.1, seed=42)
    ref = F.CodebookReferenceStepper(cfg, codes, books, B, Tn, **kw)
    dev = F.CodebookDeviceStepper(cfg, codes, books, B, Tn, **kw)
    tc.codebook_image(dev)
    for k in codes:
        assert dev.codebooks()[k].tobytes() == books[k].tobytes()
    rng = np.random.RandomState(4)
    h0, c0 = rng.normal(0, 0.3, (B, 64)).astype(np.float32), rng.normal(0, 0.3, (B, 64)).astype(np.float32)
    ref.set_state(h0, c0)
    dev.set_state(h0, c0)
    x, y = _batch(600, B, Tn, 3)
    ce_ref, ce_dev = ref.step(x, y), dev.step(x, y)
    assert abs(ce_ref - ce_dev) <= 1e-5, (ce_ref, ce_dev)
    want, got = ref.codebook_grads(), dev.codebook_grads()
    worst = {k: float(np.abs(got[k] - want[k]).max() / np.abs(want[k]).max()) for k in want}
    print("worst relative codebook-gradient deviation per tensor: %s" % {k: "%.1e" % v for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= 1e-4, (k, v)
    tc.codebook_image(dev)
    assert any(dev.codebooks()[k].tobytes() != books[k].tobytes() for k in codes)
    for k in codes:
        assert np.array_equal(dev.codes()[k], codes[k])


# ---- 10. twenty steps
@pytest.mark.parametrize("mode,bit,lr", [("tied", 3, 1e-3), ("vtable", 8, 5e-3)])
def test_twenty_steps(mode, bit, lr):
    cfg, codes, books = _model(mode, bit)
    B, Tn, K = 32, 10, 1 << bit
    kw = dict(lr=lr, dropout=0.9, norm_weight=0.1, seed=7)
    ref, dev = F.CodebookReferenceStepper(cfg, codes, books, B, Tn, **kw), F.CodebookDeviceStepper(cfg, codes, books, B, Tn, **kw)
    for i in range(20):
        x, y = _batch(600, B, Tn, 100 + i)
        ref.step_async(x, y)
        dev.step_async(x, y)
    a, b = ref.losses(), dev.losses()
    print("largest |ce_dev - ce_ref| over 20 steps: %.2e" % np.abs(a - b).max())
    assert np.abs(a - b).max() <= 1e-5
    br, bd = ref.codebooks(), dev.codebooks()
    drift = {k: float(np.abs(br[k].astype(np.float64) - bd[k]).max()) for k in br}
    print("codebook drift after 20 steps in units of lr:", {k: "%.2e" % (v / lr) for k, v in drift.items()})
    n_empty = 0
    for k, v in drift.items():
        assert v <= 20 * lr * 1e-3, (k, v)
        empty = np.bincount(codes[k].reshape(-1), minlength=K) == 0
        assert bd[k][empty].tobytes() == books[k][empty].tobytes(), k
        assert np.any(bd[k][~empty] != books[k][~empty]), k
        n_empty += int(empty.sum())
    assert (n_empty > 0) == (bit == 8)
    tc.codebook_image(dev)


# ---- 11, 12. the driver
BIT = 3
RUN = dict(lr=1e-3, max_epochs=2, dropout=1.0)


def _copy_experiment(exp):
    new = T.next_experiment_id()
    shutil.copytree(os.path.join(jconfig.experiment_path, str(exp)), os.path.join(jconfig.experiment_path, str(new)))
    return new


def _dump(exp, name="lstm_weights_comp_dump.pkl"):
    with open(os.path.join(W.weights_dir(exp), "comp_%d" % BIT, name), "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def finetuned():
    """the case of tests/test_finetune_cpu.py: the tied model trained by the numpy stepper on the Markov corpus, compressed at 3 bits by
    the compressor's restatement; then fine-tuned on the device, two epochs at lr 1e-3, dropout off"""
    root = tempfile.mkdtemp(prefix="jlm_finetune_gpu_")
    _train, _dev_ids, test = tc.write_markov_corpus(root)
    p = tc.driver_parameters("tied")
    base = T.train_experiment(p, root=root, log=lambda s: None, stepper="reference")
    with open(os.path.join(W.weights_dir(base), "lstm_weights.pkl"), "rb") as f:
        w = pickle.load(f)
    dump = {k: compress.kmeans_reference(v, BIT, seed=0) for k, v in w.items()}
    compress.write_compressed(base, BIT, dump, False)
    exp = _copy_experiment(base)
    result = F.finetune_experiment(exp, BIT, RUN, root=root, log=lambda s: None)
    return dict(root=root, base=base, exp=exp, result=result, p=p, test=test, dump=dump)


def test_two_runs_write_the_same_bytes(finetuned):
    jconfig.set_root(finetuned["root"])
    again = _copy_experiment(finetuned["base"])
    r = F.finetune_experiment(again, BIT, RUN, root=finetuned["root"], log=lambda s: None)
    assert r["saved"] and finetuned["result"]["saved"]
    assert _dump(again) == _dump(finetuned["exp"])
    assert _dump(again) != _dump(finetuned["base"])
    assert _dump(again, "lstm_weights_comp_dump.kmeans.pkl") == _dump(finetuned["base"])
    assert r["history"] == finetuned["result"]["history"]


def test_driver_on_the_device(finetuned):
    from jlm_amd import perplexity
    from jlm_amd.decoder import Decoder
    from jlm_amd.model import LSTM_Model
    from oracle import jlm_oracle as orc
    from tests.test_gpu_decode import _check_nbest
    root, exp, got, p = finetuned["root"], finetuned["exp"], finetuned["result"], finetuned["p"]
    jconfig.set_root(root)
    want = F.finetune_experiment(_copy_experiment(finetuned["base"]), BIT, RUN, root=root, log=lambda s: None, stepper="reference")
    print("validation perplexity, k-means -> epochs: device %.4f -> %s, restatement %.4f -> %s" % (
        got["kmeans_valid_pp"], [round(v, 4) for _t, v in got["history"]], want["kmeans_valid_pp"], [round(v, 4) for _t, v in want["history"]]))
    assert got["saved"] and want["saved"]
    assert abs(got["kmeans_valid_pp"] - want["kmeans_valid_pp"]) <= 1e-4 * want["kmeans_valid_pp"]
    assert abs(got["best_valid_pp"] - want["best_valid_pp"]) <= 1e-4 * want["best_valid_pp"]
    assert got["best_valid_pp"] <= 0.99 * got["kmeans_valid_pp"]
    after = pickle.loads(_dump(exp))
    for k, (code, _book) in finetuned["dump"].items():
        assert after[k][0].tobytes() == code.tobytes()
    decoded = W.load_weights(exp, BIT, p)
    for k, (code, book) in after.items():
        assert decoded[k].tobytes() == np.take(book, code).tobytes()
    model = LSTM_Model(exp, comp=BIT)
    pp, _total, _n = perplexity.stream_perplexity(model, finetuned["test"], p["batch_size"], p["num_steps"])
    print("test perplexity: fine-tuning %.6f, scoring path %.6f" % (got["best_test_pp"], pp))
    assert abs(pp - got["best_test_pp"]) <= 2e-5 * got["best_test_pp"]
    sents = synth.make_ragged_sentences(5, 3, 10, seed=42, alphabet=12)
    d = Decoder(exp, comp=BIT)
    assert len(d.model.dev.seg_codes) == d.model.dev.n_segs                 # the resident (code, codebook) path
    outs = d.decode_batch(sents, beam_width=5)
    oracle = orc.OracleDecoder(root, exp)
    oracle.model = orc.OracleLM(oracle.config, decoded)
    for s, out in zip(sents, outs):
        _check_nbest(out, oracle.decode(s, beam_width=5), ("fine-tuned", s), len(s))
