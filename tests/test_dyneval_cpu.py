"""CPU-only: dynamic evaluation's definition (jlm_amd.dyneval.DynEvalReferenceStepper) against a three-line restatement of both
rules, its degenerate forms (lam = 0 is plain SGD; zero rates are the evaluation pass), restore, the gradient statistics, the trial
on the toy model (tests/dyneval_cases.py), every refusal, and the command line on the float64 stepper."""
import os
import tempfile

import numpy as np
import pytest

from jlm_amd import config as jconfig, dyneval as DE, perplexity, train as T       # noqa: E402
from jlm_amd.score import stream_layout                                          # noqa: E402
from tests import dyneval_cases as dc, train_cases as tc                          # noqa: E402

B, TN = 3, 4


def _model(mode):
    cfg = tc.odd_cfg(mode, True)
    return cfg, T.init_weights(cfg, None, 101)


def _stats(cfg, w, seed=9):
    """statistics of the model's shapes with a few exact zeros among them"""
    rng = np.random.RandomState(seed)

    def draw(a):
        r = np.abs(rng.normal(0, 1e-2, np.shape(a))).astype(np.float32)
        r.reshape(-1)[::7] = 0.0
        return r
    return T._map(w, draw)


@pytest.mark.parametrize("mode", ["tied", "vtable", "dsoftmax"])
@pytest.mark.parametrize("rule,lr,lam,eps", [("sgd", 0.05, 0.0, 1e-3), ("sgd", 0.005, 0.02, 1e-3), ("rms", 1e-3, 0.02, 1e-3), ("rms", 3e-4, 0.9, 1e-5)])
def test_update_is_the_restated_rule(mode, rule, lr, lam, eps):
    cfg, w = _model(mode)
    stats = _stats(cfg, w) if rule == "rms" else None
    spec = DE.DynEvalSpec(lr, lam, rule, eps, B, TN)
    st = DE.DynEvalReferenceStepper(cfg, w, spec, stats)
    plain = T.ReferenceStepper(cfg, w, B, TN, lr=lr, dropout=1.0, norm_weight=0.0)
    mean = dc.flat_mean(stats) if stats is not None else None
    want = {k: a.astype(np.float64) for k, a in tc.flat_items(w)}
    theta0 = {k: a.copy() for k, a in want.items()}
    rms = {k: a.astype(np.float64) for k, a in tc.flat_items(stats)} if stats is not None else {}
    for i in range(3):
        x, y = tc.batch(tc.ODD_V, B, TN, 40 + i)
        ce = st.step(x, y)
        if i == 0:                                           # the gradient is that of the plain ce without dropout, whatever cfg's self_norm says
            assert ce == plain.step(x, y)
            for (k, a), (_k, b) in zip(tc.flat_items(st.grads()), tc.flat_items(plain.grads())):
                assert np.array_equal(a, b), k
        g = dict(tc.flat_items(st.grads()))
        for k in want:
            want[k] = dc.restated(rule, want[k], g[k], theta0[k], rms.get(k), mean, lr, lam, eps)
        got = dict(tc.flat_items(st.w))
        for k in want:
            assert np.abs(got[k] - want[k]).max() <= 1e-12, (i, k)
    assert st.t == 3


def test_sgd_without_decay_is_plain_sgd():
    cfg, w = _model("vtable")
    st = DE.DynEvalReferenceStepper(cfg, w, DE.DynEvalSpec(0.03, 0.0, "sgd", 1e-3, B, TN))
    x, y = tc.batch(tc.ODD_V, B, TN, 3)
    st.step(x, y)
    for (k, a), (_k, g), (_k2, a0) in zip(tc.flat_items(st.w), tc.flat_items(st.grads()), tc.flat_items(w)):
        assert np.array_equal(a, a0.astype(np.float64) - 0.03 * g), k


@pytest.mark.parametrize("rule", ["sgd", "rms"])
def test_zero_rates_are_the_evaluation_pass(rule):
    cfg, w = _model("dsoftmax")
    stats = _stats(cfg, w) if rule == "rms" else None
    st = DE.DynEvalReferenceStepper(cfg, w, DE.DynEvalSpec(0.0, 0.0, rule, 1e-3, B, TN), stats)
    ev = T.ReferenceStepper(cfg, w, B, TN, lr=1e-3, dropout=1.0, norm_weight=0.0)
    stream = np.random.RandomState(2).randint(0, tc.ODD_V, 200)
    pp_eval = T.run_epoch(ev, stream, B, TN, False)
    pp, total, n_tok = DE.run_stream(st, stream)
    assert np.array_equal(st.losses(), ev.losses()) and len(st.losses()) == 16
    assert n_tok == 16 * B * TN and pp == pytest.approx(pp_eval, rel=1e-15) and total == pytest.approx(np.log(pp_eval) * n_tok, rel=1e-12)
    for (k, a), (_k, a0) in zip(tc.flat_items(st.w), tc.flat_items(w)):
        assert np.array_equal(a, a0.astype(np.float64)), k


def test_restore_gives_theta0_back():
    cfg, w = _model("vtable")
    st = DE.DynEvalReferenceStepper(cfg, w, DE.DynEvalSpec(0.05, 0.01, "sgd", 1e-3, B, TN))
    for i in range(3):
        st.step(*tc.batch(tc.ODD_V, B, TN, i))
    assert any(not np.array_equal(a, a0.astype(np.float64)) for (_k, a), (_k2, a0) in zip(tc.flat_items(st.w), tc.flat_items(w)))
    st.restore()
    for (k, a), (_k, a0) in zip(tc.flat_items(st.weights()), tc.flat_items(w)):
        assert a.dtype == np.float32 and a.tobytes() == a0.tobytes(), k
    st.step(*tc.batch(tc.ODD_V, B, TN, 0))                  # and theta0 itself was not touched by the steps or by restore
    st.restore()
    for (k, a), (_k, a0) in zip(tc.flat_items(st.weights()), tc.flat_items(w)):
        assert a.tobytes() == a0.tobytes(), k


@pytest.mark.parametrize("mode", ["tied", "vtable", "dsoftmax"])
def test_gradient_stats_are_the_root_mean_square_of_the_gradients(mode):
    cfg, w = _model(mode)
    stream = np.random.RandomState(4).randint(0, tc.ODD_V, 100)
    st = DE.DynEvalReferenceStepper(cfg, w, DE.DynEvalSpec(0.5, 0.0, "sgd", 1e-3, B, TN))      # a rate that would move the weights
    got = DE.gradient_stats(st, stream, 5)
    hand = T.ReferenceStepper(cfg, w, B, TN, lr=0.0, dropout=1.0, norm_weight=0.0)
    hand._update = lambda g: None                                                          # fixed weights, the state carried
    x, y = stream_layout(stream, B, TN)
    sq = None
    for i in range(5):
        hand.step_async(x[:, i * TN:(i + 1) * TN], y[:, i * TN:(i + 1) * TN], True)
        g = {k: a.copy() for k, a in tc.flat_items(hand.grads())}
        sq = {k: g[k] ** 2 + (sq[k] if sq else 0.0) for k in g}
    for k, a in tc.flat_items(got):
        assert a.dtype == np.float32 and np.array_equal(a, np.sqrt(sq[k] / 5).astype(np.float32)), k
    for (k, a), (_k, a0) in zip(tc.flat_items(st.weights()), tc.flat_items(w)):
        assert a.tobytes() == a0.tobytes(), k                                              # no update happened
    assert not st.h.any() and len(st._losses) == 0                                         # and the state is zero again
    # mean(RMS) runs over every parameter and nothing else
    n = sum(a.size for _k, a in tc.flat_items(w))
    assert n == sum(int(np.prod(s)) for _k, _i, s, _f in T.weight_shapes(cfg))
    assert DE.mean_rms(got) == pytest.approx(dc.flat_mean(got), rel=1e-14)
    with pytest.raises(ValueError):
        DE.gradient_stats(st, stream, 9)                                                   # the stream has 8 chunks


def test_trial_on_the_toy_model():
    """The trial of DESIGN.md section 23.  This test's own run (float64 stepper, B = 1, T = 5, 3 000 tokens):
         shifted    static 1686.98 -> sgd lr 0.05 lam 0: 122.19
         in-domain  static 6.4251  -> sgd lr 0.005 lam 0.02: 6.2913;  sgd lr 0.05 lam 0: 12.78 (the divergent setting)"""
    cfg, w = dc.trial_model()
    inside, shifted = dc.streams()

    def pp(stream, lr, lam):
        return DE.run_stream(DE.DynEvalReferenceStepper(cfg, w, DE.DynEvalSpec(lr, lam)), stream)[0]
    static_in, static_sh = pp(inside, 0.0, 0.0), pp(shifted, 0.0, 0.0)
    dyn_in, dyn_sh, hot_in = pp(inside, 0.005, 0.02), pp(shifted, 0.05, 0.0), pp(inside, 0.05, 0.0)
    print("shifted: static %.2f -> %.2f; in-domain: static %.4f -> %.4f (lr 0.05, lam 0: %.4f)" % (static_sh, dyn_sh, static_in, dyn_in, hot_in))
    assert dyn_sh < static_sh / 5
    assert dyn_in < static_in
    assert hot_in > static_in                                # what the documentation warns of


# ---- refusals
BAD_SPECS = [dict(lr=float("nan")), dict(lr=float("inf")), dict(lr=-1e-3), dict(lr="0.1"), dict(lr=0.1, lam=1.0), dict(lr=0.1, lam=-0.1),
             dict(lr=0.1, eps=0.0), dict(lr=0.1, eps=-1.0), dict(lr=0.1, rule="adam"), dict(lr=0.1, rule="rms"), dict(lr=0.1, batch_size=0),
             dict(lr=0.1, num_steps=0)]


@pytest.mark.parametrize("kw", BAD_SPECS, ids=[str(k) for k in BAD_SPECS])
def test_refusals_before_any_file(kw):
    """a root that does not exist: a refusal that came after the first file access would be a FileNotFoundError"""
    nowhere = os.path.join(tempfile.gettempdir(), "jlm_dyneval_no_such_root")
    assert not os.path.exists(nowhere)
    with pytest.raises(ValueError):
        DE.check_spec(DE.DynEvalSpec(**kw))
    with pytest.raises(ValueError):
        DE.dynamic_perplexity(1, np.arange(50), DE.DynEvalSpec(**kw), root=nowhere, stepper="reference")
    with pytest.raises(ValueError):
        DE.dynamic_perplexity(1, np.arange(50), DE.DynEvalSpec(0.1), root=nowhere, stepper="reference", comp=3)
    with pytest.raises(ValueError):
        DE.dynamic_perplexity(1, np.arange(50), DE.DynEvalSpec(0.1), root=nowhere, stepper="device")
    with pytest.raises(ValueError):
        DE.dynamic_perplexity(1, np.arange(50), (0.1, 0.0), root=nowhere, stepper="reference")
    assert not os.path.exists(nowhere)


def test_refusals_of_statistics_and_untied_models():
    """statistics that are not the model's are refused once the configuration is known: before the weights are read (the experiment
    here has none) and before any stepper exists"""
    cfg, w = _model("vtable")
    root = tempfile.mkdtemp(prefix="jlm_dyneval_cpu_")
    jconfig.set_root(root)
    T.write_experiment(1, cfg, None)                        # config.json only
    good = _stats(cfg, w)
    wrong_shape = dict(good, PM=good["PM"][:, :-1])
    missing = {k: v for k, v in good.items() if k != "VT1"}
    negative = dict(good, b2=-good["b2"] - 1.0)
    zero = T._map(good, np.zeros_like)
    for stats in (wrong_shape, missing, negative, zero, [1.0]):
        with pytest.raises(ValueError):
            DE.dynamic_perplexity(1, np.arange(50), DE.DynEvalSpec(1e-3, 0.02, "rms"), stats=stats, root=root, stepper="reference")
        with pytest.raises(ValueError):
            DE.check_spec(DE.DynEvalSpec(1e-3, 0.02, "rms"), cfg, stats)
        with pytest.raises(ValueError):
            DE.DynEvalReferenceStepper(cfg, w, DE.DynEvalSpec(1e-3, 0.02, "rms"), stats)
    with pytest.raises(FileNotFoundError):                   # the good ones get as far as the weights, which are not there
        DE.dynamic_perplexity(1, np.arange(50), DE.DynEvalSpec(1e-3, 0.02, "rms"), stats=good, root=root, stepper="reference")
    untied = dict(cfg, share_embedding=False)
    with pytest.raises(NotImplementedError):
        DE.DynEvalReferenceStepper(untied, w, DE.DynEvalSpec(0.1))
    T.write_experiment(2, untied, None)
    with pytest.raises(NotImplementedError):
        DE.dynamic_perplexity(2, np.arange(50), DE.DynEvalSpec(0.1), root=root, stepper="reference")


# ---- the driver, tuning and the command line, on a written corpus
@pytest.fixture(scope="module")
def corpus():
    root = tempfile.mkdtemp(prefix="jlm_dyneval_cli_")
    _train, dev, test = tc.write_markov_corpus(root, n_train=1232, n_dev=332, n_test=332)
    cfg, w = dc.trial_model()
    return root, dc.write_experiment(root, cfg, w), dev, test


def test_driver_and_tune(corpus):
    root, exp, dev, test = corpus
    cfg, w = dc.trial_model()
    spec = DE.DynEvalSpec(0.005, 0.02, batch_size=2, num_steps=5)
    pp, total, n_tok = DE.dynamic_perplexity(exp, test, spec, root=root, stepper="reference")
    want = DE.run_stream(DE.DynEvalReferenceStepper(cfg, w, spec), test)
    assert (pp, total, n_tok) == want and n_tok == (len(test) // 2 - 1) // 5 * 5 * 2 and pp == pytest.approx(np.exp(total / n_tok))
    made = []

    def factory(c, weights, s, stats):
        made.append(DE.DynEvalReferenceStepper(c, weights, s, stats))
        return made[-1]
    grid, best = DE.tune(exp, dev, [0.0, 0.005], [0.0, 0.02], batch_size=2, root=root, stepper=factory)
    assert len(made) == 1 and grid.shape == (2, 2)          # one stepper, every point a pass of its own from theta0
    for i, lr in enumerate([0.0, 0.005]):
        for j, lam in enumerate([0.0, 0.02]):
            alone = DE.dynamic_perplexity(exp, dev, DE.DynEvalSpec(lr, lam, batch_size=2), root=root, stepper="reference")[0]
            assert grid[i, j] == alone, (lr, lam)
    assert grid[0, 0] == grid[0, 1] and best == ([0.0, 0.005][int(np.argmin(grid) // 2)], [0.0, 0.02][int(np.argmin(grid) % 2)])
    stats = DE.experiment_stats(exp, test, 500, 2, 5, root=root, stepper="reference")      # more chunks asked for than there are
    rms_pp = DE.dynamic_perplexity(exp, test, DE.DynEvalSpec(3e-4, 0.02, "rms", batch_size=2), stats=stats, root=root, stepper="reference")[0]
    assert np.isfinite(rms_pp) and rms_pp != pp


def test_command_line(corpus, capsys):
    root, exp, _dev, _test = corpus
    base = ["--root", root, "-e", str(exp), "--num_steps", "5"]
    perplexity.main(base + ["--dynamic", "--de-lr", "0.005", "--de-lam", "0.02"], de_stepper="reference")
    out = [ln for ln in capsys.readouterr().out.splitlines() if "perplexity" in ln]
    assert len(out) == 2 and out[0].startswith("Test perplexity: ") and out[1].startswith("Test perplexity with dynamic evaluation (rule sgd lr 0.005 lam 0.02 chunks of 1 x 5; ")
    static, dynamic = float(out[0].split(": ")[1]), float(out[1].rsplit(": ", 1)[1])
    test_ids = _test                                         # the stream as the file encodes it
    assert static == DE.dynamic_perplexity(exp, test_ids, DE.DynEvalSpec(0.0), root=root, stepper="reference")[0]
    assert dynamic == DE.dynamic_perplexity(exp, test_ids, DE.DynEvalSpec(0.005, 0.02), root=root, stepper="reference")[0]
    perplexity.main(base + ["--dynamic", "--de-rule", "rms", "--de-lr", "3e-4", "--de-stat-chunks", "20", "-b", "2", "--tune-dynamic",
                            os.path.join(root, "data", "dev.txt"), "--de-lrs", "1e-4,3e-4", "--de-lams", "0.02"], de_stepper="reference")
    out = capsys.readouterr().out.splitlines()
    assert any(ln.startswith("Dynamic evaluation tuned on ") and " over 2 x 1 pairs)" in ln for ln in out)
    assert out[-1].startswith("Test perplexity with dynamic evaluation (rule rms lr ") and "chunks of 2 x 5" in out[-1]


@pytest.mark.parametrize("extra", [["--cache", "10"], ["--ranks"], ["--mode", "sentence"], ["--comp", "3"], ["--de-lam", "1.0"], ["--de-lr", "-1"],
                                   ["--de-rule", "adam"], ["--de-eps", "0"], ["--de-steps", "0"], ["--tune-dynamic", "x", "--de-lrs", ""]])
def test_command_line_refusals(extra, capsys):
    with pytest.raises(SystemExit):
        perplexity.main(["--root", os.path.join(tempfile.gettempdir(), "jlm_dyneval_no_such_root"), "--dynamic"] + extra, de_stepper="reference")
    capsys.readouterr()
    with pytest.raises(SystemExit):                          # and a tuning file without --dynamic
        perplexity.main(["--tune-dynamic", "x"], de_stepper="reference")
    capsys.readouterr()
