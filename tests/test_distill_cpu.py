"""CPU-only: the numpy restatement of the distilling step (jlm_amd.distill.DistillReferenceStepper) against torch autograd on the loss
in this file's own words, its two degenerate forms (alpha = 0; a teacher that is the student), the driver and the files it writes, the
refusals, and the command line."""
import json
import os
import tempfile

import numpy as np
import pytest

from jlm_amd import config as jconfig, distill as D, train as T, weights as W       # noqa: E402
from tests import train_cases as tc                                                # noqa: E402

V, B, TN = 157, 7, 5                                         # B T = 35: no multiple of any tile size
STUDENT_SEGS = [(20, 0, 40), (9, 40, 93), (5, 93, None)]
TEACHER_SEGS = [(14, 0, 64), (6, 64, None)]                  # other cuts than the student's


def _student(mode, self_norm, n_out=None, char_rnn=False):
    cfg = tc.small_cfg(mode, V, 24, 20, self_norm, char_rnn=char_rnn, segs=STUDENT_SEGS)
    return cfg, T.init_weights(cfg, n_out, seed=11)


def _teacher(mode, n_out=None, char_rnn=False):
    if mode == "vtable":
        cfg = tc.small_cfg("vtable", V, 31, 14, True, char_rnn=char_rnn, segs=TEACHER_SEGS)
    else:
        cfg = tc.small_cfg("tied", V, 18, 27, False, char_rnn=char_rnn)
    w = T.init_weights(cfg, n_out, seed=23)
    return cfg, {k: (a * 3.0).astype(np.float32) for k, a in w.items()}          # a teacher with opinions: logits of some spread


def _inputs(n_words, H_s, H_t, seed):
    rng = np.random.RandomState(seed)
    x, y = rng.randint(0, n_words, (B, TN)), rng.randint(0, n_words, (B, TN))
    return x, y, rng.normal(0, 0.5, (B, H_s)), rng.normal(0, 0.5, (B, H_s)), rng.normal(0, 0.5, (B, H_t)), rng.normal(0, 0.5, (B, H_t))


# ---- the loss in this file's words: torch, float64, rows in time-major order
def _torch_logits(cfg, weights, ids, h0, c0, m_in, m_out, grad):
    import torch
    f64 = torch.float64
    n_out = np.asarray(weights["b2"]).shape[0]
    leaves = {}

    def leaf(key, idx=None):
        a = weights[key] if idx is None else weights[key][idx]
        leaves[(key, idx)] = torch.tensor(np.asarray(a, dtype=np.float64), dtype=f64, requires_grad=grad)
        return leaves[(key, idx)]

    segs = [(s[0], s[1], n_out if s[2] is None else s[2]) for s in cfg["embedding_seg"]]
    if cfg["V_table"]:
        emb = torch.cat([leaf("LM0")] + [leaf("LM%d" % i) @ leaf("VT%d" % i) for i in range(1, len(segs))], dim=0)
    elif cfg["D_softmax"]:
        emb = torch.block_diag(*[leaf("LM", i) for i in range(len(segs))])
    else:
        emb = leaf("LM")
    Hm = torch.cat([leaf("HM" + g) for g in "ifog"], dim=1)
    Im = torch.cat([leaf("IM" + g) for g in "ifog"], dim=1)
    bias = torch.cat([leaf("b" + g) for g in "ifog"])
    H = Hm.shape[0]
    h, c = torch.tensor(np.asarray(h0, dtype=np.float64)), torch.tensor(np.asarray(c0, dtype=np.float64))
    x = emb[torch.as_tensor(ids)] * torch.tensor(m_in)
    outs = []
    for t in range(TN):
        z = h @ Hm + x[t * B:(t + 1) * B] @ Im + bias
        i, f, o, g = torch.sigmoid(z[:, :H]), torch.sigmoid(z[:, H:2 * H]), torch.sigmoid(z[:, 2 * H:3 * H]), torch.tanh(z[:, 3 * H:])
        c = c * f + g * i
        h = torch.tanh(c) * o
        outs.append(h)
    r = torch.cat(outs, dim=0) * torch.tensor(m_out)
    return r @ leaf("PM") @ emb.t() + leaf("b2"), leaves


def _autograd(cfg, w, tcfg, tw, x, y, hs, cs, ht, ct, keep, seed, norm_weight, alpha, tau):
    """-> (ce, kl, gradients of alpha-mixed loss, dump-shaped)"""
    import torch
    ids, tgt = np.ascontiguousarray(x.T).reshape(-1), np.ascontiguousarray(y.T).reshape(-1)
    N = B * TN
    E_s = T.model_dims(cfg, np.asarray(w["b2"]).shape[0])["E"]
    E_t = T.model_dims(tcfg, np.asarray(tw["b2"]).shape[0])["E"]
    m_in = T.dropout_mask(seed, 0, T.SITE_INPUT, (N, E_s), keep)
    m_out = T.dropout_mask(seed, 0, T.SITE_OUTPUT, (N, cfg["hidden_size"]), keep)
    ys, leaves = _torch_logits(cfg, w, ids, hs, cs, m_in, m_out, True)
    with torch.no_grad():
        yt, _ = _torch_logits(tcfg, tw, ids, ht, ct, np.ones((N, E_t)), np.ones((N, tcfg["hidden_size"])), False)
    lse = torch.logsumexp(ys, dim=1)
    ce = (lse - ys[torch.arange(N), torch.as_tensor(tgt)]).mean()
    log_q = torch.log_softmax(yt / tau, dim=1)
    log_p = torch.log_softmax(ys / tau, dim=1)
    kl = torch.nn.functional.kl_div(log_p, log_q, reduction="none", log_target=True).sum(dim=1).mean()
    loss = (1.0 - alpha) * ce + alpha * tau * tau * kl + norm_weight * (lse * lse).mean()
    loss.backward()
    grads = {}
    for (key, idx), t in leaves.items():
        if idx is None:
            grads[key] = t.grad.numpy()
        else:
            grads.setdefault(key, {})[idx] = t.grad.numpy()
    return float(ce.detach()), float(kl.detach()), {k: [v[i] for i in sorted(v)] if isinstance(v, dict) else v for k, v in grads.items()}


def _check_against_autograd(cfg, w, tcfg, tw, self_norm, keep, alpha, tau, seed=77):
    n_out = np.asarray(w["b2"]).shape[0]
    x, y, hs, cs, ht, ct = _inputs(n_out, cfg["hidden_size"], tcfg["hidden_size"], 5)
    st = D.DistillReferenceStepper(cfg, w, tcfg, tw, B, TN, lr=1e-3, dropout=keep, norm_weight=0.1, seed=seed, alpha=alpha, temperature=tau)
    st.set_state(hs, cs)
    st.set_teacher_state(ht, ct)
    ce = st.step(x, y)
    ce_t, kl_t, g_t = _autograd(cfg, w, tcfg, tw, x, y, hs, cs, ht, ct, keep, seed, 0.1 if self_norm else 0.0, alpha, tau)
    assert abs(ce - ce_t) <= 1e-12 * max(1.0, abs(ce_t))
    assert len(st.kls()) == 1 and abs(st.kls()[0] - kl_t) <= 1e-12 * max(1.0, abs(kl_t))
    assert kl_t > 1e-3                                       # the soft term is there to be checked
    got, want = dict(tc.flat_items(st.grads())), dict(tc.flat_items(g_t))
    assert sorted(got) == sorted(want)
    for k in want:
        scale = np.abs(want[k]).max()
        assert scale > 0, k
        assert np.abs(got[k] - want[k]).max() <= 1e-9 * scale, (k, np.abs(got[k] - want[k]).max() / scale)


@pytest.mark.parametrize("student", ["tied", "vtable", "dsoftmax"])
@pytest.mark.parametrize("teacher", ["vtable", "tied"])
@pytest.mark.parametrize("tau", [1.0, 2.5])
@pytest.mark.parametrize("alpha", [0.3, 1.0])
@pytest.mark.parametrize("self_norm", [False, True])
def test_distill_gradients_equal_autograd(student, teacher, tau, alpha, self_norm):
    cfg, w = _student(student, self_norm)
    tcfg, tw = _teacher(teacher)
    _check_against_autograd(cfg, w, tcfg, tw, self_norm, 0.9, alpha, tau)


def test_distill_gradients_character_models():
    """a character pair: both softmaxes run over n_out = 37 characters, not over vocab_size words"""
    cfg, w = _student("tied", True, n_out=37, char_rnn=True)
    tcfg, tw = _teacher("tied", n_out=37, char_rnn=True)
    assert w["b2"].shape == (37,) and tw["b2"].shape == (37,)
    _check_against_autograd(cfg, w, tcfg, tw, True, 0.9, 0.3, 2.5)


def test_teacher_state_is_carried_and_reset():
    """two training steps: the second starts the teacher from where the first left it; reset_state zeroes it"""
    cfg, w = _student("tied", False)
    tcfg, tw = _teacher("vtable")
    x, y, *_ = _inputs(V, 24, 31, 8)
    st = D.DistillReferenceStepper(cfg, w, tcfg, tw, B, TN, dropout=1.0, alpha=0.5, temperature=2.0)
    st.step(x, y)
    ids = np.ascontiguousarray(x.T).reshape(-1)
    _y, h1, c1 = D.teacher_forward(st.tw, st.td, ids, np.zeros((B, 31)), np.zeros((B, 31)), B, TN)
    assert np.array_equal(st.th, h1) and np.array_equal(st.tc, c1) and np.abs(h1).max() > 0
    st.step(x, y, train=False)                               # an evaluation step does not run the teacher
    assert np.array_equal(st.th, h1) and len(st.kls()) == 1
    st.step(x, y)
    _y, h2, c2 = D.teacher_forward(st.tw, st.td, ids, h1, c1, B, TN)
    assert np.array_equal(st.th, h2) and not np.array_equal(h2, h1)
    st.reset_state()
    assert not st.th.any() and not st.tc.any() and len(st.kls()) == 0


# ---- the degenerate forms
@pytest.mark.parametrize("mode", ["tied", "vtable", "dsoftmax"])
def test_alpha_zero_is_the_plain_step(mode):
    cfg, w = _student(mode, True)
    tcfg, tw = _teacher("vtable")
    kw = dict(lr=1e-3, dropout=0.9, norm_weight=0.1, seed=5)
    plain = T.ReferenceStepper(cfg, w, B, TN, **kw)
    st = D.DistillReferenceStepper(cfg, w, tcfg, tw, B, TN, alpha=0.0, temperature=2.5, **kw)
    for i in range(3):
        x, y = tc.batch(V, B, TN, 40 + i)
        plain.step_async(x, y)
        st.step_async(x, y)
    assert np.array_equal(plain.losses(), st.losses()) and len(st.kls()) == 0
    a, b = dict(tc.flat_items(plain.w)), dict(tc.flat_items(st.w))
    for k in a:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("alpha,tau", [(0.3, 1.0), (1.0, 2.5), (0.5, 2.0)])
def test_a_teacher_that_is_the_student_teaches_nothing(alpha, tau):
    """keep = 1 and the student's own weights as the teacher: kl = 0 and the soft term vanishes, so the gradient is (1 - alpha) times the
    hard gradient plus the self-normalisation term, which alpha does not scale"""
    cfg, w = _student("vtable", True)
    x, y, hs, cs, _ht, _ct = _inputs(V, 24, 24, 6)
    kw = dict(lr=1e-3, dropout=1.0, seed=5)

    def grads(stepper):
        stepper.set_state(hs, cs)
        stepper.step(x, y)
        return dict(tc.flat_items(stepper.grads()))
    st = D.DistillReferenceStepper(cfg, w, cfg, w, B, TN, norm_weight=0.1, alpha=alpha, temperature=tau, **kw)
    st.set_teacher_state(hs, cs)
    got = grads(st)
    assert abs(st.kls()[0]) <= 1e-12
    both = grads(T.ReferenceStepper(cfg, w, B, TN, norm_weight=0.1, **kw))               # hard + self-norm
    hard = grads(T.ReferenceStepper(dict(cfg, self_norm=False), w, B, TN, norm_weight=0.1, **kw))
    for k in got:
        want = (1.0 - alpha) * hard[k] + (both[k] - hard[k])
        assert np.abs(got[k] - want).max() <= 1e-12 * np.abs(both[k]).max(), k


# ---- the driver
@pytest.fixture(scope="module")
def corpus_root():
    root = tempfile.mkdtemp(prefix="jlm_distill_cpu_")
    tc.write_markov_corpus(root, n_train=2032, n_dev=432, n_test=432)
    teacher = T.train_experiment(tc.driver_parameters("vtable", self_norm=True, max_epochs=1), root=root, log=lambda s: None,
                                 stepper="reference")
    return root, teacher


def _folder_bytes(path):
    out = {}
    for base, _dirs, files in os.walk(path):
        for fn in files:
            with open(os.path.join(base, fn), "rb") as f:
                out[os.path.relpath(os.path.join(base, fn), path)] = f.read()
    return out


def test_driver_writes_an_ordinary_experiment(corpus_root):
    root, teacher = corpus_root
    tdir = os.path.join(jconfig.experiment_path, str(teacher))
    before = _folder_bytes(tdir)
    p = tc.driver_parameters("tied", hidden_size=32, embed_size=16, max_epochs=2)
    lines = []
    exp = D.distill_experiment(teacher, p, alpha=0.5, temperature=2.0, root=root, log=lines.append, stepper=D.DistillReferenceStepper)
    assert _folder_bytes(tdir) == before and before                      # the teacher's folder is only read
    assert any(s.startswith("Validation perplexity") for s in lines)
    plain = T.train_experiment(p, root=root, log=lambda s: None, stepper="reference")
    mine, theirs = (_folder_bytes(os.path.join(jconfig.experiment_path, str(e))) for e in (exp, plain))
    assert mine["config.json"] == theirs["config.json"]
    assert sorted(mine) == sorted(list(theirs) + ["distill.json"])
    assert json.loads(mine["distill.json"]) == dict(teacher_id=teacher, alpha=0.5, temperature=2.0, teacher_hidden_size=64,
                                                    teacher_embed_size=32, teacher_softmax="V_table")
    w = W.load_weights(exp, 0, jconfig.load_config_dict(exp))
    assert w["LM"].shape == (tc.MARKOV_V, 16) and w["HMi"].shape == (32, 32) and w["LM"].dtype == np.float32
    assert np.isfinite(D.last_result["best_valid_pp"]) and len(D.last_result["history"]) == 2
    assert D.distill_experiment(teacher, p, root=root, log=lambda s: None, stepper="reference") == plain + 1


def _refused(root, exc, *args, **kw):
    listing = sorted(os.listdir(jconfig.experiment_path))
    with pytest.raises(exc) as e:
        D.distill_experiment(*args, root=root, log=lambda s: None, stepper="reference", **kw)
    assert sorted(os.listdir(jconfig.experiment_path)) == listing       # before any file is made
    return str(e.value)


def test_refusals_come_before_any_file(corpus_root):
    root, teacher = corpus_root
    jconfig.set_root(root)
    p = tc.driver_parameters("tied", hidden_size=32, embed_size=16, max_epochs=1)
    for alpha in (-0.1, 1.5, float("nan"), "0.5", None, True):
        assert "alpha" in _refused(root, ValueError, teacher, p, alpha=alpha)
    for tau in (0.0, -1.0, float("inf"), float("nan"), "2"):
        assert "temperature" in _refused(root, ValueError, teacher, p, temperature=tau)
    assert "does not exist" in _refused(root, ValueError, 987, p)
    # teachers written by hand, each wrong in one way
    base = jconfig.load_config_dict(teacher)
    good = W.load_weights(teacher, 0, base)
    other = T.init_weights(dict(base, vocab_size=500), None, 3)
    nxt = T.next_experiment_id()
    T.write_experiment(nxt, base, other)                                              # 500 output words
    T.write_experiment(nxt + 1, dict(base, char_rnn=True), good)                      # a character teacher for a word student
    T.write_experiment(nxt + 2, dict(base, share_embedding=False), good)              # an untied teacher
    assert "output words" in _refused(root, ValueError, nxt, p)
    assert "character" in _refused(root, ValueError, nxt + 1, p)
    assert "character" in _refused(root, ValueError, teacher, dict(p, char_rnn=True))
    assert "share_embedding" in _refused(root, ValueError, nxt + 2, p)
    # check_parameters' own refusals pass through unchanged
    _refused(root, ValueError, teacher, dict(p, class_based=True))
    _refused(root, ValueError, teacher, dict(p, optimizer="rmsprop"))
    _refused(root, NotImplementedError, teacher, dict(p, share_embedding=False))
    assert "unknown" in _refused(root, ValueError, teacher, dict(p, alpha=0.5))
    assert "alpha" not in T.DEFAULTS and "temperature" not in T.DEFAULTS and "teacher" not in T.DEFAULTS


def test_cli_takes_every_train_flag_and_three_more():
    ap = D.build_parser()
    argv = ["--root", "/x", "--teacher", "7", "--alpha", "0.25", "--temperature", "3"]
    for k, v in T.DEFAULTS.items():
        argv += ["--" + k, json.dumps(v) if isinstance(v, list) else str(v)]
    args = vars(ap.parse_args(argv))
    assert (args.pop("root"), args.pop("teacher"), args.pop("alpha"), args.pop("temperature")) == ("/x", "7", 0.25, 3.0)
    assert set(args) == set(T.DEFAULTS)
    for k, v in T.DEFAULTS.items():
        assert args[k] == ([list(s) for s in v] if isinstance(v, list) else v), k
    d = ap.parse_args(["--teacher", "3"])
    assert (d.alpha, d.temperature) == (0.5, 1.0)
    with pytest.raises(SystemExit):
        ap.parse_args([])                                    # --teacher is required
