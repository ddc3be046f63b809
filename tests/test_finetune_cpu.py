"""CPU: fine-tuning the codebooks of a compressed model (jlm_amd.finetune) without a GPU: the host tables of the device stepper, the
numpy float64 stepper against torch autograd, the weight accessors, the driver on the Markov corpus, the refusals, the exports."""
import os
import pickle
import tempfile

import numpy as np
import pytest

from jlm_amd import _lib, compress, config as jconfig, finetune as F, train as T, weights as W
from tests import train_cases as tc

SEGS = [(20, 0, 40), (9, 40, 93), (5, 93, None)]
V, H, E = 157, 24, 20


def _random_model(mode, bit, self_norm=False, seed=5):
    """a small model as (cfg, codes, books): random codes (at 8 bits the 24-element biases leave most codes empty), codebooks drawn at
    the scale of the Glorot weights"""
    cfg = tc.small_cfg(mode, V, H, E, self_norm, segs=SEGS)
    rng = np.random.RandomState(seed)
    K = 1 << bit
    codes, books = {}, {}
    for key, _idx, shape, fan in T.weight_shapes(cfg):
        codes[key] = rng.randint(0, K, shape).astype(np.uint8)
        books[key] = rng.uniform(-1, 1, (K, 1)).astype(np.float32) * np.float32(T.glorot_limit(fan))
    return cfg, codes, books


def _layout(cfg):
    """DeviceStepper's flat layout, restated: the gate matrices side by side, every tensor at a multiple of 4 elements"""
    layout, off = [], 0
    shapes = [("HM", None, (H, 4 * H)), ("IM", None, (E, 4 * H)), ("b", None, (4 * H,))]
    shapes += [(k, i, s) for k, i, s, _f in T.weight_shapes(cfg) if k[:2] not in ("HM", "IM") and k not in ("bi", "bf", "bo", "bg")]
    for key, idx, shape in shapes:
        n = int(np.prod(shape))
        layout.append((key, idx, shape, off, n))
        off += (n + 3) // 4 * 4
    return layout, off


# ---- 1. the group builder
@pytest.mark.parametrize("mode", ["tied", "vtable"])
@pytest.mark.parametrize("bit,chunk", [(3, F.CODEBOOK_CHUNK), (3, 100), (8, 7)])
def test_group_builder(mode, bit, chunk):
    cfg, codes, _books = _random_model(mode, bit)
    K = 1 << bit
    names = F.tensor_names(cfg)
    layout, n_flat = _layout(cfg)
    gid, order, chunks = F.build_groups(layout, names, codes, K, n_flat, chunk)
    assert gid.dtype == np.int32 and order.dtype == np.int32 and chunks.dtype == np.int32 and gid.shape == (n_flat,)
    covered = np.zeros(n_flat, dtype=bool)
    for key, _idx, shape, off, n in layout:
        covered[off:off + n] = True
        a = gid[off:off + n].reshape(shape)
        if key in ("HM", "IM", "b"):                     # the four codebooks of the gate tensors land on their column ranges
            for k, g in enumerate("ifog"):
                t = names.index(key + g)
                assert np.array_equal(a[..., k * H:(k + 1) * H], t * K + codes[key + g].astype(np.int64)), (key, g)
        else:
            assert np.array_equal(a, names.index(key) * K + codes[key].astype(np.int64)), key
    assert any(n % 4 for _k, _i, _s, _o, n in layout) and not covered.all()       # the case has padding
    assert np.array_equal(gid == -1, ~covered)
    assert np.array_equal(np.sort(order), np.nonzero(covered)[0])                # every coded element exactly once
    keys = gid[order].astype(np.int64) * n_flat + order
    assert np.all(np.diff(keys) > 0)                                             # sorted by (gid, offset)
    grp, begin, length = chunks[:, 0], chunks[:, 1], chunks[:, 2]
    assert length.min() >= 1 and length.max() <= chunk
    assert np.all(np.diff(grp) >= 0)
    assert begin[0] == 0 and np.array_equal(begin[1:], (begin + length)[:-1]) and begin[-1] + length[-1] == len(order)
    for c in range(len(chunks)):
        assert np.all(gid[order[begin[c]:begin[c] + length[c]]] == grp[c])
    counts = np.bincount(gid[covered], minlength=len(names) * K)
    assert np.array_equal(np.bincount(grp, weights=length, minlength=len(names) * K), counts)
    assert np.array_equal(np.bincount(grp, minlength=len(names) * K), -(-counts // chunk))    # no more pieces than needed
    if chunk == 7:
        assert (counts == 0).any() and (counts > chunk).any()


# ---- 2. the codebook gradients are the per-code sums of autograd's weight gradients
@pytest.mark.parametrize("mode", ["vtable", "tied"])
@pytest.mark.parametrize("self_norm", [False, True])
@pytest.mark.parametrize("bit", [3, 8])
def test_codebook_gradients_equal_summed_autograd(mode, self_norm, bit):
    B, Tn, keep = 7, 5, 0.9
    cfg, codes, books = _random_model(mode, bit, self_norm)
    K = 1 << bit
    rng = np.random.RandomState(5)
    x, y = rng.randint(0, V, (B, Tn)), rng.randint(0, V, (B, Tn))
    h0, c0 = rng.normal(0, 0.5, (B, H)), rng.normal(0, 0.5, (B, H))
    st = F.CodebookReferenceStepper(cfg, codes, books, B, Tn, lr=1e-3, dropout=keep, norm_weight=0.1, seed=77)
    st.set_state(h0, c0)
    w = st.weights()
    for k in codes:
        assert np.array_equal(w[k], np.take(books[k], codes[k]))
    ce = st.step(x, y, train=True)
    m_in = T.dropout_mask(77, 0, T.SITE_INPUT, (B * Tn, st.d["E"]), keep)
    m_out = T.dropout_mask(77, 0, T.SITE_OUTPUT, (B * Tn, H), keep)
    ce_t, g_t, _state = tc.torch_grads(cfg, w, x, y, h0, c0, m_in, m_out, 0.1 if self_norm else 0.0)
    assert abs(ce - ce_t) <= 1e-12 * max(1.0, abs(ce_t))
    got = st.codebook_grads()
    assert sorted(got) == sorted(codes)
    some_empty = False
    for k in codes:
        want = np.zeros(K)
        np.add.at(want, codes[k].reshape(-1), g_t[k].reshape(-1))
        scale = np.abs(want).max()
        assert scale > 0, k
        assert got[k].shape == (K, 1)
        assert np.abs(got[k][:, 0] - want).max() <= 1e-9 * scale, k
        empty = np.bincount(codes[k].reshape(-1), minlength=K) == 0
        assert np.all(got[k][empty, 0] == 0.0)
        some_empty |= bool(empty.any())
    assert some_empty == (bit == 8)


# ---- 3. five steps
@pytest.mark.parametrize("mode", ["tied", "vtable"])
def test_five_steps_keep_the_weights_a_codebook_image(mode):
    B, Tn, bit = 7, 5, 8
    cfg, codes, books = _random_model(mode, bit, True)
    K = 1 << bit
    st = F.CodebookReferenceStepper(cfg, codes, books, B, Tn, lr=5e-3, dropout=0.9, norm_weight=0.1, seed=3)
    rng = np.random.RandomState(9)
    for _ in range(5):
        st.step_async(rng.randint(0, V, (B, Tn)), rng.randint(0, V, (B, Tn)))
    assert np.isfinite(st.losses()).all() and st.t == 5
    w, b, c = st.weights(), st.codebooks(), st.codes()
    moved = 0
    for k in codes:
        assert c[k].dtype == np.uint8 and np.array_equal(c[k], codes[k])
        assert b[k].dtype == np.float32 and b[k].shape == (K, 1) and w[k].dtype == np.float32
        assert np.array_equal(w[k], np.take(b[k], c[k]))
        empty = np.bincount(codes[k].reshape(-1), minlength=K) == 0
        assert np.array_equal(b[k][empty], books[k][empty])
        moved += int((b[k][~empty] != books[k][~empty]).sum())
    assert moved > 0
    st.load_weights(w)
    again = st.codebooks()
    for k in codes:
        assert np.array_equal(again[k], b[k])
    k = "PM"
    shared = int(np.argmax(np.bincount(codes[k].reshape(-1), minlength=K)))             # a code that several elements carry
    i, j = np.nonzero(codes[k].reshape(-1) == shared)[0][:2]
    bad = {n: a.copy() for n, a in w.items()}
    bad[k].reshape(-1)[j] += np.float32(1.0)
    assert i != j
    with pytest.raises(ValueError):
        st.load_weights(bad)
    bad = {n: a.copy() for n, a in w.items()}
    bad[k] = bad[k][:-1]
    with pytest.raises(ValueError):
        st.load_weights(bad)


# ---- 4. the driver with the numpy stepper on the Markov corpus
BIT = 3


def _file_bytes(exp):
    out = {}
    wdir = W.weights_dir(exp)
    for d, _dirs, files in os.walk(wdir):
        for fn in files:
            with open(os.path.join(d, fn), "rb") as f:
                out[os.path.relpath(os.path.join(d, fn), wdir)] = f.read()
    return out


@pytest.fixture(scope="module")
def compressed_experiment():
    root = tempfile.mkdtemp(prefix="jlm_finetune_cpu_")
    tc.write_markov_corpus(root)
    p = tc.driver_parameters("tied")
    exp = T.train_experiment(p, root=root, log=lambda s: None, stepper="reference")
    with open(os.path.join(W.weights_dir(exp), "lstm_weights.pkl"), "rb") as f:
        w = pickle.load(f)
    dump = {k: compress.kmeans_reference(v, BIT, seed=0) for k, v in w.items()}
    compress.write_compressed(exp, BIT, dump, False)
    return root, exp, p, dump


def test_driver_reference_improves_on_kmeans(compressed_experiment):
    """Measured (tied model, 3 bits, lr 1e-3, dropout off): validation perplexity 7.5019 with the k-means codebooks, 7.3306 and 7.2970
    after the two epochs (2.7 % better; the numpy prototype that preceded this module gave 7.502, 7.331, 7.297); test 7.1853."""
    root, exp, p, dump = compressed_experiment
    jconfig.set_root(root)
    before = _file_bytes(exp)
    lines = []
    r = F.finetune_experiment(exp, BIT, dict(lr=0.0, max_epochs=1, dropout=1.0), root=root, log=lines.append, stepper="reference")
    assert not r["saved"] and r["best_valid_pp"] == r["kmeans_valid_pp"] and _file_bytes(exp) == before       # lr 0: nothing is written
    assert any(s.startswith("Validation perplexity (k-means): ") for s in lines)
    r = F.finetune_experiment(exp, BIT, dict(lr=1e-3, max_epochs=2, dropout=1.0), root=root, log=lambda s: None, stepper="reference")
    valid = [v for _t, v in r["history"]]
    print("validation perplexity: k-means %.4f, epochs %s; test %.4f" % (r["kmeans_valid_pp"], ["%.4f" % v for v in valid], r["best_test_pp"]))
    assert sorted(r) == ["best_test_pp", "best_valid_pp", "history", "kmeans_valid_pp", "saved", "test_pp"]
    assert r["saved"] and len(valid) == 2
    assert r["best_valid_pp"] <= 0.99 * r["kmeans_valid_pp"]
    assert valid[0] < r["kmeans_valid_pp"] and valid[1] < valid[0] and r["best_valid_pp"] == valid[1]
    # on disk
    cdir = os.path.join(W.weights_dir(exp), "comp_%d" % BIT)
    with open(os.path.join(cdir, "lstm_weights_comp_dump.pkl"), "rb") as f:
        after = pickle.load(f)
    with open(os.path.join(cdir, "lstm_weights_comp_dump.kmeans.pkl"), "rb") as f:
        backup = pickle.load(f)
    decoded = W.load_weights(exp, BIT, p)
    assert list(after) == list(dump) and sorted(decoded) == sorted(dump)
    changed = 0
    for k, (code, book) in dump.items():
        assert after[k][0].dtype == code.dtype and np.array_equal(after[k][0], code)
        assert after[k][1].dtype == np.float32 and after[k][1].shape == book.shape
        assert decoded[k].dtype == np.float32 and np.array_equal(decoded[k], np.take(after[k][1], after[k][0]))
        assert np.array_equal(backup[k][0], code) and np.array_equal(backup[k][1], book)
        changed += int((after[k][1] != book).sum())
    assert changed > 0
    assert not any(fn.endswith(".txt") for fn in os.listdir(cdir))                  # there were no text dumps: none appear
    # a second run starts from the fine-tuned codebooks and does not touch the backup
    with open(os.path.join(cdir, "lstm_weights_comp_dump.kmeans.pkl"), "rb") as f:
        kept = f.read()
    r2 = F.finetune_experiment(exp, BIT, dict(lr=1e-3, max_epochs=1, dropout=1.0), root=root, log=lambda s: None, stepper="reference")
    assert abs(r2["kmeans_valid_pp"] - r["best_valid_pp"]) <= 1e-6 * r["best_valid_pp"]
    with open(os.path.join(cdir, "lstm_weights_comp_dump.kmeans.pkl"), "rb") as f:
        assert f.read() == kept


def test_text_dumps_follow_when_they_were_there():
    """write_compressed is compress_experiment's writer: with the text dumps present before, a save rewrites them too"""
    root = tempfile.mkdtemp(prefix="jlm_finetune_cpu_")
    tc.write_markov_corpus(root, n_train=2032, n_dev=432, n_test=432)
    p = tc.driver_parameters("vtable", max_epochs=1)
    exp = T.train_experiment(p, root=root, log=lambda s: None, stepper="reference")
    with open(os.path.join(W.weights_dir(exp), "lstm_weights.pkl"), "rb") as f:
        w = pickle.load(f)
    compress.write_compressed(exp, 2, {k: compress.kmeans_reference(v, 2, seed=0) for k, v in w.items()}, True)
    r = F.finetune_experiment(exp, 2, dict(lr=1e-3, max_epochs=1, dropout=1.0), root=root, log=lambda s: None, stepper="reference")
    assert r["saved"]
    cdir = os.path.join(W.weights_dir(exp), "comp_2")
    with open(os.path.join(cdir, "lstm_weights_comp_dump.pkl"), "rb") as f:
        after = pickle.load(f)
    for k, (code, book) in after.items():
        assert np.array_equal(np.loadtxt(os.path.join(cdir, k + "_codebook.txt"), dtype=np.float32), book.reshape(-1))
        assert np.array_equal(np.loadtxt(os.path.join(cdir, k + "_code.txt"), dtype=np.int64), code)


# ---- 5. the refusals, each before any file is touched
def _write_experiment(root, cfg, dump, bit, exp=1):
    jconfig.set_root(root)
    T.write_experiment(exp, cfg, None)
    if dump is not None:
        compress.write_compressed(exp, bit, dump, False)
    return exp


def _small_dump(cfg, bit, seed=1):
    w = T.init_weights(cfg, None, seed)
    return {k: compress.kmeans_reference(v, bit, seed=0) for k, v in w.items()}


@pytest.mark.parametrize("case", ["dsoftmax", "no dump", "other bit", "mixed lengths", "shape", "missing tensor", "unknown parameter"])
def test_refusals(case):
    root = tempfile.mkdtemp(prefix="jlm_finetune_cpu_")
    tc.write_markov_corpus(root, n_train=432, n_dev=132, n_test=132)
    p = T.check_parameters(tc.driver_parameters("dsoftmax" if case == "dsoftmax" else "vtable"))
    bit, params = 3, {}
    if case == "dsoftmax":
        w = T.init_weights(p, None, 1)
        dump = {k: compress.kmeans_reference(v, bit, seed=0) for k, v in w.items() if not isinstance(v, list)}
    elif case == "no dump":
        dump = None
    else:
        dump = _small_dump(p, bit)
    if case == "other bit":
        bit = 4                                           # comp_4 does not exist
        exp = _write_experiment(root, p, dump, 3)
    else:
        if case == "mixed lengths":
            dump["PM"] = compress.kmeans_reference(T.init_weights(p, None, 1)["PM"], 2, seed=0)
        if case == "shape":
            dump["LM1"] = (dump["LM1"][0][:-1], dump["LM1"][1])
        if case == "missing tensor":
            del dump["VT2"]
        if case == "unknown parameter":
            params = {"hidden_size": 32}
        exp = _write_experiment(root, p, dump, bit)
    before = _file_bytes(exp)
    called = []
    with pytest.raises(ValueError):
        F.finetune_experiment(exp, bit, params, root=root, log=lambda s: None, stepper=lambda *a, **k: called.append(1))
    assert not called and _file_bytes(exp) == before


def test_a_codebook_of_another_length_is_refused():
    """comp_3 holding 4-entry codebooks throughout: all of one length, but not 2^3"""
    root = tempfile.mkdtemp(prefix="jlm_finetune_cpu_")
    tc.write_markov_corpus(root, n_train=432, n_dev=132, n_test=132)
    p = T.check_parameters(tc.driver_parameters("tied"))
    exp = _write_experiment(root, p, _small_dump(p, 2), 3)
    with pytest.raises(ValueError):
        F.finetune_experiment(exp, 3, root=root, log=lambda s: None, stepper="reference")


# ---- 6. exports and the command line
def test_exports_and_command_line():
    assert "jlm_train_expand_codes" in _lib.EXPORTS and "jlm_train_codebook_grad" in _lib.EXPORTS
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "jlm_hip.h")) as f:
        assert "#define JLM_CODEBOOK_CHUNK %d\n" % F.CODEBOOK_CHUNK in f.read()
    a = F.build_parser().parse_args(["--root", "R", "-e", "7", "-c", "3", "--lr", "0.002", "--max_epochs", "2", "--early_stopping", "0",
                                     "--batch_size", "16", "--num_steps", "5", "--dropout", "1.0", "--tf_random_seed", "9"])
    assert (a.root, a.experiment, a.comp) == ("R", "7", 3)
    assert (a.lr, a.max_epochs, a.early_stopping, a.batch_size, a.num_steps, a.dropout, a.tf_random_seed) == (0.002, 2, 0, 16, 5, 1.0, 9)
    b = F.build_parser().parse_args(["-e", "7", "-c", "3"])
    assert all(getattr(b, k) is None for k in F.OVERRIDES)
