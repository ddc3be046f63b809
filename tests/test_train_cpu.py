"""CPU-only: the numpy restatement of the training step (jlm_amd.train.ReferenceStepper) against torch autograd, Adam, the dropout
mask, the initial weights, the driver (epochs, early stopping, the files written) and the command line."""
import json
import math
import os
import pickle
import tempfile

import numpy as np
import pytest

from jlm_amd import config as jconfig, model as jmodel, synth, train as T, weights as W       # noqa: E402
from tests import train_cases as tc                                                          # noqa: E402

MODES = ("tied", "vtable", "dsoftmax")


def _step_inputs(V, B, Tn, H, seed):
    rng = np.random.RandomState(seed)
    x = rng.randint(0, V, (B, Tn))
    y = rng.randint(0, V, (B, Tn))
    h0 = rng.normal(0, 0.5, (B, H))
    c0 = rng.normal(0, 0.5, (B, H))
    return x, y, h0, c0


# ---- 1. the backward pass is the gradient
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("self_norm", [False, True])
@pytest.mark.parametrize("keep", [0.9, 1.0])
def test_reference_gradients_equal_autograd(mode, self_norm, keep):
    V, H, E, B, Tn = 157, 24, 20, 7, 5                       # B T = 35: no multiple of any tile size
    cfg = tc.small_cfg(mode, V, H, E, self_norm, segs=[(20, 0, 40), (9, 40, 93), (5, 93, None)])
    w = T.init_weights(cfg, None, seed=11)
    x, y, h0, c0 = _step_inputs(V, B, Tn, H, 5)
    st = T.ReferenceStepper(cfg, w, B, Tn, lr=1e-3, dropout=keep, norm_weight=0.1, seed=77)
    st.set_state(h0, c0)
    ce = st.step(x, y, train=True)
    d = st.d
    m_in = T.dropout_mask(77, 0, T.SITE_INPUT, (B * Tn, d["E"]), keep)
    m_out = T.dropout_mask(77, 0, T.SITE_OUTPUT, (B * Tn, H), keep)
    ce_t, g_t, (h_t, c_t) = tc.torch_grads(cfg, w, x, y, h0, c0, m_in, m_out, 0.1 if self_norm else 0.0)
    assert abs(ce - ce_t) <= 1e-12 * max(1.0, abs(ce_t))
    np.testing.assert_allclose(st.h, h_t, rtol=0, atol=1e-12)
    np.testing.assert_allclose(st.c, c_t, rtol=0, atol=1e-12)
    got = dict(tc.flat_items(st.grads()))
    want = dict(tc.flat_items(g_t))
    assert sorted(got) == sorted(want)
    for k in want:
        scale = np.abs(want[k]).max()
        assert scale > 0, k
        assert np.abs(got[k] - want[k]).max() <= 1e-9 * scale, k


def test_reference_gradients_character_model():
    """a character model only changes the softmax rows: n_out = len(CharVocab) instead of vocab_size"""
    cfg = tc.small_cfg("tied", 600, 24, 12, True, char_rnn=True)
    n_out = 37
    w = T.init_weights(cfg, n_out, seed=3)
    assert w["LM"].shape == (n_out, 12) and w["b2"].shape == (n_out,)
    x, y, h0, c0 = _step_inputs(n_out, 6, 4, 24, 9)
    st = T.ReferenceStepper(cfg, w, 6, 4, dropout=0.9, norm_weight=0.1, seed=5)
    st.set_state(h0, c0)
    st.step(x, y)
    m_in = T.dropout_mask(5, 0, T.SITE_INPUT, (24, 12), 0.9)
    m_out = T.dropout_mask(5, 0, T.SITE_OUTPUT, (24, 24), 0.9)
    _ce, g_t, _s = tc.torch_grads(cfg, w, x, y, h0, c0, m_in, m_out, 0.1)
    got, want = dict(tc.flat_items(st.grads())), dict(tc.flat_items(g_t))
    for k in want:
        assert np.abs(got[k] - want[k]).max() <= 1e-9 * np.abs(want[k]).max(), k


# ---- 2. Adam
def test_adam_reference_is_tensorflows_formula():
    rng = np.random.RandomState(0)
    w = rng.normal(size=50)
    m, v = np.zeros(50), np.zeros(50)
    w2, m2, v2 = w.copy(), m.copy(), v.copy()
    lr = 5e-3
    for t in range(1, 6):
        g = rng.normal(size=50)
        w, m, v = T.adam_reference(w, g, m, v, t, lr)
        lr_t = lr * math.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)
        m2 = 0.9 * m2 + (1 - 0.9) * g
        v2 = 0.999 * v2 + (1 - 0.999) * g * g
        w2 = w2 - lr_t * m2 / (np.sqrt(v2) + 1e-8)
        np.testing.assert_allclose(w, w2, rtol=0, atol=1e-15)
        np.testing.assert_allclose(m, m2, rtol=0, atol=1e-15)
        np.testing.assert_allclose(v, v2, rtol=0, atol=1e-15)
    for t in (1, 2, 1000):
        assert abs(T.adam_lr_t(lr, t) - lr * math.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)) <= 1e-18


# ---- 3. the dropout mask
def test_dropout_mask_is_a_pure_function():
    a = T.dropout_mask(9, 4, 0, (33, 17), 0.9)
    assert np.array_equal(a, T.dropout_mask(9, 4, 0, (33, 17), 0.9))
    assert set(np.unique(a)) <= {0.0, 1 / 0.9}
    assert not np.array_equal(a, T.dropout_mask(9, 5, 0, (33, 17), 0.9))
    assert not np.array_equal(a, T.dropout_mask(9, 4, 1, (33, 17), 0.9))
    assert not np.array_equal(a, T.dropout_mask(10, 4, 0, (33, 17), 0.9))
    pieces = [T.dropout_mask(9, 4, 0, (r1 - r0, 17), 0.9, offset=r0 * 17) for r0, r1 in ((0, 5), (5, 6), (6, 33))]
    assert np.array_equal(a, np.concatenate(pieces, axis=0))
    assert np.array_equal(T.dropout_mask(9, 4, 0, (8, 8), 1.0), np.ones((8, 8)))


@pytest.mark.parametrize("keep", [0.9, 0.5])
def test_dropout_mask_kept_fraction(keep):
    n = 1 << 20
    frac = float((T.dropout_mask(123, 0, 1, (n,), keep) != 0).mean())
    assert abs(frac - keep) <= 5 * math.sqrt(keep * (1 - keep) / n)


# ---- 4. the initial weights
@pytest.mark.parametrize("mode", MODES)
def test_init_weights_shapes_limits_determinism(mode):
    cfg = tc.small_cfg(mode, 600, 64, 32, False)
    for n_out in (None, 451):
        want = synth.make_weights(cfg, n_out=n_out)
        got = T.init_weights(cfg, n_out, seed=101)
        assert sorted(got) == sorted(want)
        for (k, a), (_k, b) in zip(tc.flat_items(got), tc.flat_items(want)):
            assert a.shape == b.shape and a.dtype == np.float32, k
        for key, idx, shape, fan in T.weight_shapes(cfg, n_out):
            a = got[key] if idx is None else got[key][idx]
            lim = T.glorot_limit(fan)
            assert np.abs(a).max() <= lim and np.abs(a).max() > 0.5 * lim, key
        again = T.init_weights(cfg, n_out, seed=101)
        other = T.init_weights(cfg, n_out, seed=102)
        assert all(np.array_equal(a, b) for (_k, a), (_k2, b) in zip(tc.flat_items(got), tc.flat_items(again)))
        assert not np.array_equal(got["PM"], other["PM"])
    assert T.glorot_limit((64,)) == math.sqrt(6.0 / 128) and T.glorot_limit((32, 64)) == math.sqrt(6.0 / 96)


# ---- 5. the driver
@pytest.fixture(scope="module")
def corpus_root():
    root = tempfile.mkdtemp(prefix="jlm_train_cpu_")
    streams = tc.write_markov_corpus(root)
    return root, streams


@pytest.mark.parametrize("mode", ["tied", "vtable"])
def test_driver_learns_the_markov_corpus(corpus_root, mode):
    """Measured (Glorot limits, dropout 0.9, four epochs; the add-one unigram perplexity of the dev cut as the files encode it is 439.1,
    a quarter of it 109.8), validation perplexity per epoch: tied 57.09, 10.49, 7.17, 6.13; V_table 60.88, 18.90, 13.22, 10.94."""
    root, (train, dev, _test) = corpus_root
    uni = tc.unigram_perplexity(train, dev)
    lines = []
    exp = T.train_experiment(tc.driver_parameters(mode), root=root, log=lines.append, stepper="reference")
    res = dict(T.last_result)
    valid = [v for _t, v in res["history"]]
    print("unigram perplexity %.1f, validation perplexities %s" % (uni, valid))
    assert len(valid) == 4
    assert all(b < a for a, b in zip(valid, valid[1:])), valid
    assert valid[-1] < uni / 4, (valid[-1], uni)
    assert [l for l in lines if l.startswith("Epoch ")] == ["Epoch %d" % i for i in range(4)]
    assert any(l.startswith("Training perplexity: ") for l in lines) and any(l.startswith("Validation perplexity: ") for l in lines)
    assert any(l.startswith("Test perplexity: ") for l in lines)
    # the experiment loads
    jconfig.set_root(root)
    cfg = jconfig.load_config_dict(exp)
    assert cfg["embed_size"] == 32 and cfg["hidden_size"] == 64 and cfg["V_table"] == (mode == "vtable")
    raw = W.load_weights(exp, 0, cfg)
    w, embed, _blocks, _vt = jmodel.prepare_weights(cfg, raw)
    assert w["LM"].shape == (600, 32) and w["PM"].shape == (64, 32) and w["HMi"].shape == (64, 64) and w["b2"].shape == (600,)
    assert all(np.asarray(a).dtype == np.float32 for _k, a in tc.flat_items(raw))


def test_experiment_ids_count_up(corpus_root):
    root, _ = corpus_root
    jconfig.set_root(root)
    first = T.next_experiment_id()
    os.makedirs(os.path.join(jconfig.experiment_path, str(first + 3)))
    assert T.next_experiment_id() == first + 4


class ScriptedStepper:
    """returns a scripted perplexity per pass (the three corpora are told apart by their ids); its weights name the epoch they were
    read in"""

    def __init__(self, valid_pp, test_pp):
        self.valid_pp, self.test_pp = list(valid_pp), list(test_pp)
        self.epoch, self.kind, self.n_steps, self.loaded = -1, None, 0, None

    def reset_state(self):
        self.n_steps, self.kind = 0, None

    def step_async(self, x, y, train=True):
        if self.n_steps == 0:
            self.kind = {1: "train", 2: "dev", 3: "test"}[int(x[0, 0])]
            assert train == (self.kind == "train")
            if self.kind == "train":
                self.epoch += 1
            self.pp = 200.0 if self.kind == "train" else self.valid_pp[self.epoch] if self.kind == "dev" else self.test_pp.pop(0)
        self.n_steps += 1

    def losses(self):
        return np.full(self.n_steps, math.log(self.pp))

    def weights(self):
        return {"epoch": np.array([self.epoch], dtype=np.float32)}

    def load_weights(self, w):
        self.loaded = w


def test_early_stopping_saves_the_best_epoch():
    train, dev, test = (np.full(500, k, dtype=np.int32) for k in (1, 2, 3))
    st = ScriptedStepper([100.0, 80.0, 90.0, 85.0, 70.0, 60.0], [50.0, 60.0])
    saved = []
    res = T.fit(st, train, dev, test, dict(batch_size=4, num_steps=5, max_epochs=6, early_stopping=1), log=lambda s: None,
                save=lambda w: saved.append(w))
    # epoch 1 is the best; epoch 3 is the first with epoch - best > 1: the run stops there, before the better epochs 4 and 5
    assert res["best_epoch"] == 1 and res["last_epoch"] == 3 and len(res["history"]) == 4
    assert abs(res["best_valid_pp"] - 80.0) < 1e-9
    assert [float(w["epoch"][0]) for w in saved] == [0.0, 1.0]
    assert float(res["best_weights"]["epoch"][0]) == 1.0 and st.loaded is res["best_weights"]
    assert abs(res["test_pp"] - 50.0) < 1e-9 and abs(res["best_test_pp"] - 60.0) < 1e-9


def test_weights_on_disk_are_the_best_epochs(corpus_root):
    """the file holds what the stepper's weights were at the last improvement of the validation perplexity, as float32"""
    root, _ = corpus_root
    snaps = []

    class Recording(T.ReferenceStepper):
        def weights(self):
            snaps.append(T.ReferenceStepper.weights(self))
            return snaps[-1]
    p = tc.driver_parameters("tied", max_epochs=2, early_stopping=0, dropout=1.0)
    exp = T.train_experiment(p, root=root, log=lambda s: None, stepper=Recording)
    res = dict(T.last_result)
    with open(os.path.join(jconfig.experiment_path, str(exp), "weights", "lstm_weights.pkl"), "rb") as f:
        disk = pickle.load(f)
    assert sorted(disk) == sorted(synth.make_weights(tc.small_cfg("tied")))
    valid = [v for _t, v in res["history"]]
    assert len(snaps) == sum(1 for i, v in enumerate(valid) if v < min([float("inf")] + valid[:i]))
    assert all(np.array_equal(disk[k], snaps[-1][k]) and disk[k].dtype == np.float32 for k in disk)
    with open(os.path.join(jconfig.experiment_path, str(exp), "config.json")) as f:
        assert json.load(f)["lr"] == 5e-3


def test_vtable_config_keeps_embed_size(corpus_root):
    root, _ = corpus_root
    p = tc.driver_parameters("vtable", max_epochs=1, embed_size=48)
    exp = T.train_experiment(p, root=root, log=lambda s: None, stepper="reference")
    jconfig.set_root(root)
    cfg = jconfig.load_config_dict(exp)
    assert cfg["embed_size"] == 48                    # un-mutated: the model's E is embedding_seg[0][0] = 32
    raw = W.load_weights(exp, 0, cfg)
    assert raw["PM"].shape == (64, 32) and raw["LM1"].shape == (210, 16) and raw["VT1"].shape == (16, 32)
    w, _e, blocks, v_tables = jmodel.prepare_weights(cfg, raw)
    assert w["LM"].shape == (600, 32) and len(blocks) == 3


# ---- 6. the command line and the compat shim
def test_cli_parses_every_reference_key():
    ap = T.build_parser()
    argv = ["--root", "/x"]
    for k, v in T.DEFAULTS.items():
        argv += ["--" + k, json.dumps(v) if isinstance(v, list) else str(v)]
    args = vars(ap.parse_args(argv))
    assert args.pop("root") == "/x"
    assert set(args) == set(T.DEFAULTS)
    for k, v in T.DEFAULTS.items():
        assert args[k] == ([list(s) for s in v] if isinstance(v, list) else v), k
    assert ap.parse_args(["--V_table", "true", "--lr", "0.01"]).V_table is True


def test_unbuilt_options_are_refused_before_anything_runs():
    with pytest.raises(ValueError):
        T.train_experiment({"class_based": True}, root="/nonexistent")
    with pytest.raises(ValueError):
        T.train_experiment({"optimizer": "rmsprop"}, root="/nonexistent")
    with pytest.raises(NotImplementedError):
        T.train_experiment({"share_embedding": False}, root="/nonexistent")
    with pytest.raises(ValueError):
        T.check_parameters({"no_such_key": 1})


def test_compat_shim_exposes_parameters():
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "compat", "train", "train.py")
    spec = importlib.util.spec_from_file_location("compat_train_train", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert set(mod.parameters) == set(T.DEFAULTS) and mod.parameters["optimizer"] == "adam"
    mod.parameters["class_based"] = True
    with pytest.raises(ValueError):
        mod.train_RNNLM()


def test_non_finite_loss_names_epoch_and_step(corpus_root):
    root, _ = corpus_root
    p = tc.driver_parameters("tied", self_norm=True, max_epochs=1)      # in float64 it takes the square of an lse of 1e200 to overflow
    w = {k: np.asarray(v, dtype=np.float64) for k, v in T.init_weights(p, 600, 101).items()}
    w["PM"][3, 5] = 1e200
    with pytest.raises(T.NonFiniteLoss) as e, np.errstate(all="ignore"):
        T.train_experiment(p, root=root, log=lambda s: None, stepper="reference", initial_weights=w)
    assert e.value.epoch == 0 and e.value.step == 0


# ---- float32 against float64 at the headline sizes: what plain float32 uses of the 1e-4 gradient bar
def test_float32_deviation_at_mid_sizes():
    """Measured: 7.3e-7 (mid V_table, self-norm, dropout 0.9, B = 128, T = 20), under a hundredth of the bar; about 11 s."""
    import torch
    cfg = synth.make_config(50000, 512, 256, "vtable", synth.README_SEGS, True)
    w = T.init_weights(cfg, None, 101)
    x, y, h0, c0 = _step_inputs(50000, 128, 20, 512, 1)
    m_in = T.dropout_mask(1, 0, 0, (2560, 200), 0.9)
    m_out = T.dropout_mask(1, 0, 1, (2560, 512), 0.9)
    _c, g64, _s = tc.torch_grads(cfg, w, x, y, h0, c0, m_in, m_out, 0.1)
    _c, g32, _s = tc.torch_grads(cfg, w, x, y, h0, c0, m_in, m_out, 0.1, dtype=torch.float32)
    a, b = dict(tc.flat_items(g64)), dict(tc.flat_items(g32))
    worst = max(np.abs(a[k] - b[k]).max() / np.abs(a[k]).max() for k in a)
    print("float32 against float64, mid vtable, one step: worst per-tensor relative gradient deviation %.3e" % worst)
    assert worst < 1e-5               # plain float32 must leave nine tenths of the 1e-4 bar to the device
