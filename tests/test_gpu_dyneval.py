"""GPU: dynamic evaluation on the device (jlm_amd.dyneval.DynEvalDeviceStepper) against its definition, the float64
DynEvalReferenceStepper (pinned by tests/test_dyneval_cpu.py), on the bars the trainer is held to (tests/test_gpu_train.py,
tests/test_gpu_train_shapes.py): every gradient tensor within 1e-4 of the reference tensor's largest gradient, every chunk's ce within
1e-5, an end-to-end perplexity within 1e-4 relative.

The weights after n steps are held to  n (lr 1e-4 Gmax / d + 2^-23 max|w|)  per tensor: a step moves a weight by lr g / d (d = 1 under
sgd, RMS + eps >= min(RMS) + eps under rms), the gradient bar allows g to be off by 1e-4 Gmax (Gmax: the reference's largest gradient of
the tensor over the steps), and the float32 weight is rounded once per step, 2^-24 max|w|, with as much again for the decay term's
arithmetic.  The bound ignores that a deviation of the weights feeds back into the next gradient; at twenty steps that is second order.

Every device stepper here runs with ``split_kc=16``, so each product of 64 x 64 tiles or fewer whose contraction is 32 or longer goes
through ``train_gemm_splitk``."""
import tempfile

import numpy as np
import pytest

torch = pytest.importorskip("torch")
from jlm_amd import dyneval as DE, train as T                               # noqa: E402
from tests import dyneval_cases as dc, train_cases as tc                   # noqa: E402

pytestmark = pytest.mark.gpu
NAN = float("nan")
STEPS = 20
RULES = {"sgd": dict(lr=0.05, lam=0.02, rule="sgd"), "rms": dict(lr=1e-3, lam=0.02, rule="rms", eps=1e-3)}
MODELS = [(size, mode) for size in ("odd", "small") for mode in ("tied", "vtable", "dsoftmax")]
SHAPES = [(1, 1), (1, 5), (3, 4)]
_models, _runs = {}, {}


def _model(size, mode):
    if (size, mode) not in _models:
        cfg = tc.odd_cfg(mode, True) if size == "odd" else tc.small_cfg(mode)
        _models[(size, mode)] = (cfg, T.init_weights(cfg, None, 101))
    return _models[(size, mode)]


def _stream(cfg, n, seed):
    return np.random.RandomState(seed).randint(0, cfg["vocab_size"], n)


def _device(cfg, w, spec, stats=None, **kw):
    kw.setdefault("split_kc", 16)
    return DE.DynEvalDeviceStepper(cfg, w, spec, stats, **kw)


def _run(size, mode, B, Tn, rule):
    """STEPS chunks on both steppers, once per case: the first step's gradients, every ce, Gmax and the final weights"""
    key = (size, mode, B, Tn, rule)
    if key in _runs:
        return _runs[key]
    cfg, w = _model(size, mode)
    spec = DE.DynEvalSpec(batch_size=B, num_steps=Tn, **RULES[rule])
    stats = None
    if rule == "rms":                                         # the reference's statistics, as float32, for both
        stats = DE.gradient_stats(DE.DynEvalReferenceStepper(cfg, w, DE.DynEvalSpec(0.0, batch_size=B, num_steps=Tn)),
                                  _stream(cfg, 6 * B * Tn + B, 7), 6)
    ref, dev = DE.DynEvalReferenceStepper(cfg, w, spec, stats), _device(cfg, w, spec, stats)
    h0, c0 = tc.carried_state(B, cfg["hidden_size"], 4)
    ref.set_state(h0, c0)
    dev.set_state(h0, c0)
    out = dict(stats=stats, gmax={}, first=None)
    for i in range(STEPS):
        x, y = tc.batch(cfg["vocab_size"], B, Tn, 50 + i)
        ref.step_async(x, y)
        dev.step_async(x, y)
        g = dict(tc.flat_items(ref.grads()))
        for k, a in g.items():
            out["gmax"][k] = max(out["gmax"].get(k, 0.0), float(np.abs(a).max()))
        if i == 0:
            out["first"] = (ref.grads(), dev.grads())
    out.update(ce_ref=ref.losses(), ce_dev=dev.losses(), w_ref=T._map(ref.w, np.copy), w_dev=dev.weights(), dev=dev, ref=ref,
               part=int(dev.part.numel()))
    _runs[key] = out
    return out


CASES = [(size, mode, B, Tn) for size, mode in MODELS for B, Tn in SHAPES]
IDS = ["%s-%s-B%d-T%d" % c for c in CASES]


@pytest.mark.parametrize("size,mode,B,Tn", CASES, ids=IDS)
def test_one_step_gradients(size, mode, B, Tn):
    r = _run(size, mode, B, Tn, "sgd")
    worst = tc.worst_relative(r["first"][1], r["first"][0])
    print("worst relative gradient deviation %.2e (%s); split scratch %d words" % (max(worst.values()), max(worst, key=worst.get), r["part"]))
    for k, v in worst.items():
        assert v <= 1e-4, (k, v)
    assert r["part"] > 0, "no product of this step took the split form"


@pytest.mark.parametrize("rule", ["sgd", "rms"])
@pytest.mark.parametrize("size,mode,B,Tn", CASES, ids=IDS)
def test_twenty_steps(size, mode, B, Tn, rule):
    r = _run(size, mode, B, Tn, rule)
    dce = np.abs(r["ce_dev"] - r["ce_ref"])
    kw = RULES[rule]
    ratios = {}
    for (k, got), (_k, want) in zip(tc.flat_items(r["w_dev"]), tc.flat_items(r["w_ref"])):
        d = 1.0 if rule == "sgd" else float(dict(tc.flat_items(r["stats"]))[k].min()) + kw["eps"]
        wmax = max(float(np.abs(want).max()), float(np.abs(dict(tc.flat_items(_model(size, mode)[1]))[k]).max()))
        bound = STEPS * (kw["lr"] * 1e-4 * r["gmax"][k] / d + 2.0 ** -23 * wmax)
        ratios[k] = float(np.abs(got.astype(np.float64) - want).max()) / bound
    print("%s: worst |ce_dev - ce_ref| %.2e; worst weight deviation / bound %.3f (%s)" % (rule, dce.max(), max(ratios.values()),
                                                                                        max(ratios, key=ratios.get)))
    assert len(dce) == STEPS and dce.max() <= 1e-5
    for k, v in ratios.items():
        assert v <= 1.0, (k, v)
    assert r["dev"].t == STEPS


@pytest.mark.parametrize("size,mode", MODELS, ids=["%s-%s" % m for m in MODELS])
def test_zero_rates_restore_and_reproducibility(size, mode):
    cfg, w = _model(size, mode)
    B, Tn = 3, 4
    stream = _stream(cfg, 10 * B * Tn + B, 8)
    zero = _device(cfg, w, DE.DynEvalSpec(0.0, 0.0, batch_size=B, num_steps=Tn))
    pad = tc.padding_mask(zero.layout, zero.n_flat)
    pp, _total, n_tok = DE.run_stream(zero, stream)
    ce_zero = zero.losses()
    assert n_tok == 10 * B * Tn
    assert zero.W.cpu().numpy().tobytes() == zero.W0.cpu().numpy().tobytes(), "zero rates moved a weight"
    for (k, a), (_k, a0) in zip(tc.flat_items(zero.weights()), tc.flat_items(w)):
        assert a.tobytes() == a0.tobytes(), k
    ev = _device(cfg, w, DE.DynEvalSpec(0.0, 0.0, batch_size=B, num_steps=Tn))
    assert T.run_epoch(ev, stream, B, Tn, False) == pytest.approx(pp, rel=1e-14)
    assert ev.losses().tobytes() == ce_zero.tobytes(), "the ce of a zero-rate step is not the evaluation pass's"
    # restore, and two runs
    spec = DE.DynEvalSpec(0.05, 0.02, batch_size=B, num_steps=Tn)
    outs = []
    for poison in (False, False, True):
        dev = _device(cfg, w, spec)
        dev.reset_state()
        for i in range(4):
            if poison:
                for buf in (dev.part, dev.partial, dev.Y):
                    buf.fill_(NAN)
            dev.step_async(*tc.batch(cfg["vocab_size"], B, Tn, 70 + i))
        outs.append((dev.W.cpu().numpy().tobytes(), dev.losses().tobytes()))
        assert not dev.W.cpu().numpy()[pad].any() and not dev.G.cpu().numpy()[pad].any(), "the padding moved"
    assert outs[0] == outs[1], "two runs differ"
    assert outs[0] == outs[2], "the result depends on what part, partial or Y held"
    assert outs[0][0] != dev.W0.cpu().numpy().tobytes()
    dev.restore()
    assert dev.W.cpu().numpy().tobytes() == dev.W0.cpu().numpy().tobytes()
    for (k, a), (_k, a0) in zip(tc.flat_items(dev.weights()), tc.flat_items(w)):
        assert a.tobytes() == a0.tobytes(), k
    # with split_max_tiles=0 every product is the trainer's launch: no scratch, and the same step to the ce bar
    off = _device(cfg, w, spec, split_max_tiles=0)
    for i in range(4):
        off.step_async(*tc.batch(cfg["vocab_size"], B, Tn, 70 + i))
    assert off.part.numel() == 0 and dev.part.numel() > 0
    assert np.abs(off.losses() - np.frombuffer(outs[0][1], dtype=np.float64)).max() <= 1e-5


@pytest.mark.parametrize("size,mode", MODELS, ids=["%s-%s" % m for m in MODELS])
def test_gradient_stats_on_the_device(size, mode):
    cfg, w = _model(size, mode)
    B, Tn, n = 3, 4, 6
    stream = _stream(cfg, n * B * Tn + B, 9)
    spec = DE.DynEvalSpec(0.5, 0.0, batch_size=B, num_steps=Tn)
    ref, dev = DE.DynEvalReferenceStepper(cfg, w, spec), _device(cfg, w, spec)
    gmax = {}
    seen = ref._update

    def note(g):
        for k, a in tc.flat_items(g):
            gmax[k] = max(gmax.get(k, 0.0), float(np.abs(a).max()))
        seen(g)
    ref._update = note
    want = DE.gradient_stats(ref, stream, n)
    dev.partial.fill_(NAN)
    got = DE.gradient_stats(dev, stream, n)
    worst = {}
    for (k, a), (_k, b) in zip(tc.flat_items(got), tc.flat_items(want)):
        assert a.dtype == np.float32 and a.shape == b.shape
        worst[k] = float(np.abs(a.astype(np.float64) - b).max()) / gmax[k]
    print("worst |dRMS| / Gmax %.2e (%s); mean(RMS) on the device %.9e, from the read-back %.9e" % (
        max(worst.values()), max(worst, key=worst.get), dev.device_mean, DE.mean_rms(got)))
    for k, v in worst.items():
        assert v <= 1e-4, (k, v)
    assert abs(dev.device_mean - DE.mean_rms(got)) <= 1e-12 * DE.mean_rms(got)          # the padding is not counted
    assert dev.W.cpu().numpy().tobytes() == dev.W0.cpu().numpy().tobytes() and not dev.Hs[:B].any()
    again = DE.gradient_stats(_device(cfg, w, spec), stream, n)
    for (k, a), (_k, b) in zip(tc.flat_items(got), tc.flat_items(again)):
        assert a.tobytes() == b.tobytes(), k


def test_refusals_on_the_device():
    cfg, w = _model("odd", "vtable")
    with pytest.raises(NotImplementedError):
        DE.DynEvalDeviceStepper(dict(cfg, share_embedding=False), w, DE.DynEvalSpec(0.1))
    with pytest.raises(ValueError):
        DE.DynEvalDeviceStepper(cfg, w, DE.DynEvalSpec(0.1, rule="rms"))
    with pytest.raises(ValueError):
        DE.DynEvalDeviceStepper(cfg, w, DE.DynEvalSpec(0.1), split_kc=24)


def test_end_to_end_on_the_toy_model():
    """The trial of tests/test_dyneval_cpu.py through ``dynamic_perplexity`` on the device and on the float64 stepper: the perplexities
    agree to 1e-4 relative, and at zero rates the device's is the scoring path's (``perplexity.stream_perplexity``) to 2e-7."""
    from jlm_amd import config as jconfig, perplexity
    from jlm_amd.model import LSTM_Model
    cfg, w = dc.trial_model()
    inside, shifted = dc.streams()
    root = tempfile.mkdtemp(prefix="jlm_dyneval_gpu_")
    tc.write_markov_corpus(root, n_train=432, n_dev=132, n_test=132)          # the lexicon the scoring path's model loads
    exp = dc.write_experiment(root, cfg, w)
    figures = {}
    for name, stream, lr, lam in (("shifted", shifted, 0.05, 0.0), ("in-domain", inside, 0.005, 0.02)):
        spec = DE.DynEvalSpec(lr, lam)
        got = DE.dynamic_perplexity(exp, stream, spec, root=root)
        want = DE.dynamic_perplexity(exp, stream, spec, root=root, stepper="reference")
        static = DE.dynamic_perplexity(exp, stream, DE.DynEvalSpec(0.0), root=root)
        figures[name] = (static[0], got[0], want[0])
        print("%s: static %.4f, dynamic %.6f on the device, %.6f in float64 (relative difference %.2e)" % (
            name, static[0], got[0], want[0], abs(got[0] - want[0]) / want[0]))
        assert got[2] == want[2] == 3000
    jconfig.set_root(root)
    pp, _total, n_tok = perplexity.stream_perplexity(LSTM_Model(exp), inside, 1, 5)
    print("zero rates: %.9f; the scoring path: %.9f (relative difference %.2e)" % (figures["in-domain"][0], pp,
                                                                                 abs(pp - figures["in-domain"][0]) / pp))
    for name, (static, got, want) in figures.items():
        assert abs(got - want) <= 1e-4 * want, name
    assert figures["shifted"][1] < figures["shifted"][0] / 5 and figures["in-domain"][1] < figures["in-domain"][0]
    assert n_tok == 3000 and abs(pp - figures["in-domain"][0]) <= 2e-7 * pp


def test_command_line_on_the_device(capsys):
    """``python -m jlm_amd.perplexity --dynamic``: the static line is the scoring path's, the dynamic line ``dynamic_perplexity``'s"""
    from jlm_amd import perplexity
    cfg, w = dc.trial_model()
    root = tempfile.mkdtemp(prefix="jlm_dyneval_gpu_cli_")
    train, _dev, test = tc.write_markov_corpus(root, n_train=1232, n_dev=332, n_test=332)
    exp = dc.write_experiment(root, cfg, w)
    base = ["--root", root, "-e", str(exp), "--num_steps", "5", "-b", "2"]
    perplexity.main(base)
    plain = [ln for ln in capsys.readouterr().out.splitlines() if "perplexity" in ln]
    perplexity.main(base + ["--dynamic", "--de-rule", "rms", "--de-lr", "3e-4", "--de-stat-chunks", "20"])
    out = [ln for ln in capsys.readouterr().out.splitlines() if "perplexity" in ln]
    assert len(plain) == 1 and len(out) == 2 and out[0] == plain[0]
    assert out[1].startswith("Test perplexity with dynamic evaluation (rule rms lr 0.0003 lam 0.02 chunks of 2 x 5; ")
    stats = DE.experiment_stats(exp, train, 20, 2, 5, root=root)       # ``train``: the ids as data/train.txt encodes
    want = DE.dynamic_perplexity(exp, test, DE.DynEvalSpec(3e-4, 0.02, "rms", batch_size=2), stats=stats, root=root)[0]
    assert float(out[1].rsplit(": ", 1)[1]) == want
