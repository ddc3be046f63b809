"""GPU: distillation on the device (jlm_amd.distill.DistillDeviceStepper over csrc/jlm_train.hip's distill kernels through
torch.ops.jlm.train_distill_*) against float64: the two passes as launched, one step's gradients against DistillReferenceStepper, the
degenerate alpha = 0, the frozen teacher, twenty steps, the chunk budget, reproducibility, the driver end to end, and the non-finite path.

The bars are the training suite's (tests/test_gpu_train.py): 4 ulp of a value below 16 for a normaliser, 2e-5 s for dy -- here times
1 + alpha tau, the coefficient of the added term --, 1e-5 for ce and kl, 1e-4 relative per gradient tensor, 20 lr 1e-3 weight drift,
1e-4 / 2e-5 relative perplexity."""
import os
import pickle
import tempfile

import numpy as np
import pytest

torch = pytest.importorskip("torch")
from jlm_amd import config as jconfig, distill as D, ops as jops, synth, train as T      # noqa: E402
from tests import poison, train_cases as tc                                             # noqa: E402

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
CUTS = {1000: [(0, 384), (384, 384), (768, 232)], 1: [(0, 1)]}           # the last window of 1000 words ends inside a granule


def _dev(a, dtype=None):
    return torch.from_numpy(np.array(a, order="C")).to("cuda", dtype=dtype)          # a copy: the shared logits are read-only


def _nan(*shape, dtype=torch.float32):
    return poison.fill_tensor(torch.empty(*shape, device="cuda", dtype=dtype), poison.FILL_A)


def _lse64(y):
    mx = y.max(1)
    return mx + np.log(np.exp(y - mx[:, None]).sum(1))


_LOGITS = {}


def _logits(N, V):
    """the student's and the teacher's logits ~ N(0, 2^2), float32: made once per shape and never written to"""
    if (N, V) not in _LOGITS:
        rng = np.random.RandomState(4 + N + V)
        ys, yt = (rng.normal(0, 2.0, (N, V)).astype(np.float32) for _ in range(2))
        ys.setflags(write=False)
        yt.setflags(write=False)
        _LOGITS[(N, V)] = ys, yt
    return _LOGITS[(N, V)]


def _pass1(ys, yt, cuts, tau, ld_extra=5):
    """the three pairs after pass 1 over ``cuts``; the scratches have leading dimensions of their own and run starts as NaN"""
    N = ys.shape[0]
    width = max(n for _v0, n in cuts)
    Y, Yt = _nan(N, width), _nan(N, width + ld_extra)
    run = _nan(6, N)
    ysd, ytd = _dev(ys), _dev(yt)
    for k, (v0, n) in enumerate(cuts):
        Y[:, :n].copy_(ysd[:, v0:v0 + n])
        Yt[:, :n].copy_(ytd[:, v0:v0 + n])
        jops.backend().train_distill_lse_update(Y, width, Yt, width + ld_extra, n, N, 1.0 / tau, run, k == 0)
    return run


# ---- pass 1
@pytest.mark.parametrize("N", [37, 1])
@pytest.mark.parametrize("V", [1000, 1])
@pytest.mark.parametrize("tau", [1.0, 2.5])
def test_pass_one_normalisers(N, V, tau):
    ys, yt = _logits(N, V)
    run = _pass1(ys, yt, CUTS[V], tau)
    got = run.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()                                      # nothing of the NaN fill survives
    worst = {}
    for k, (name, y) in enumerate((("L_s", ys.astype(np.float64)), ("A_s", ys.astype(np.float64) / tau), ("A_t", yt.astype(np.float64) / tau))):
        want = _lse64(y)
        assert np.abs(want).max() < 16
        worst[name] = np.abs(got[2 * k] + np.log(got[2 * k + 1]) - want).max()
    print("N = %d, V = %d, tau = %g: worst normaliser deviations in ulp of 16: %s" % (N, V, tau, {k: "%.2f" % (v / (16 * U)) for k, v in worst.items()}))
    for name, v in worst.items():
        assert v <= 4 * U * 16, (name, v)
    if tau == 1.0:
        # the L_s pair is train_lse_update's, bit for bit, and the A_s pair is the L_s pair
        width = max(n for _v0, n in CUTS[V])
        Y, run_m, run_s = _nan(N, width), _nan(N), _nan(N)
        for k, (v0, n) in enumerate(CUTS[V]):
            Y[:, :n].copy_(_dev(ys)[:, v0:v0 + n])
            jops.backend().train_lse_update(Y, width, n, N, run_m, run_s, k == 0)
        assert torch.equal(run[0], run_m) and torch.equal(run[1], run_s)
        assert torch.equal(run[2], run[0]) and torch.equal(run[3], run[1])


@pytest.mark.parametrize("tau", [1.0, 2.5])
def test_pass_one_does_not_depend_on_the_cut(tau):
    ys, yt = _logits(37, 1000)
    assert torch.equal(_pass1(ys, yt, [(0, 1000)], tau), _pass1(ys, yt, CUTS[1000], tau))


# ---- pass 2
def _pass2(ys, yt, cuts, tau, alpha, target, nw):
    """both passes over ``cuts`` -> (dy [N, V], tgt_logit, kl_row, kl, flag): every output starts as NaN"""
    N, V = ys.shape
    O = jops.backend()
    width = max(n for _v0, n in cuts)
    run = _pass1(ys, yt, cuts, tau, ld_extra=0)
    Y, Yt = _nan(N, width), _nan(N, width)
    tgt, kl_row, kl = _nan(N), _nan(N), _nan(2, dtype=torch.float64)
    flag = torch.zeros(1, device="cuda", dtype=torch.int32)
    ysd, ytd, td = _dev(ys), _dev(yt), _dev(target)
    dy = np.zeros((N, V), dtype=np.float32)
    for k, (v0, n) in enumerate(cuts):
        Y[:, :n].copy_(ysd[:, v0:v0 + n])
        Yt[:, :n].copy_(ytd[:, v0:v0 + n])
        O.train_distill_dy(Y, width, Yt, width, n, v0, N, run, td, tgt, kl_row, 1.0 / N, 2.0 * nw, 1.0 - alpha, alpha * tau, 1.0 / tau, k == 0)
        dy[:, v0:v0 + n] = Y[:, :n].cpu().numpy()
    O.train_distill_kl(kl_row, N, kl, flag)
    return dy, tgt.cpu().numpy(), kl_row.cpu().numpy(), float(kl[0]), int(flag[0])


def _want2(ys, yt, tau, alpha, target, nw):
    N = ys.shape[0]
    y, t = ys.astype(np.float64), yt.astype(np.float64)
    Ls = _lse64(y)
    ls, lt = y / tau - _lse64(y / tau)[:, None], t / tau - _lse64(t / tau)[:, None]
    q = np.exp(lt)
    kl = np.where(q > 0, q * (lt - ls), 0.0).sum(1)
    p = np.exp(y - Ls[:, None])
    dy = (1 - alpha) * p + 2 * nw * Ls[:, None] * p + alpha * tau * (np.exp(ls) - q)
    dy[np.arange(N), target] -= 1 - alpha
    return dy / N, kl


@pytest.mark.parametrize("N", [37, 1])
@pytest.mark.parametrize("V", [1000, 1])
@pytest.mark.parametrize("tau", [1.0, 2.5])
@pytest.mark.parametrize("alpha", [0.3, 1.0])
def test_pass_two_dy_and_kl(N, V, tau, alpha):
    ys, yt = _logits(N, V)
    yt = yt.copy()
    if V > 1:
        yt[0, 5] = -200.0                                              # q underflows to 0 there: it adds 0, never 0 times -inf
    target = np.random.RandomState(9).randint(0, V, N).astype(np.int32)
    target[:4] = [0, 383, V - 1, 768][:N] if V > 1 else 0              # targets in the first and in the last window
    nw, s = 0.1, 1.0 / N
    dy, tgt, kl_row, kl, flag = _pass2(ys, yt, CUTS[V], tau, alpha, target, nw)
    want_dy, want_kl = _want2(ys, yt, tau, alpha, target, nw)
    assert np.isfinite(dy).all() and np.isfinite(tgt).all() and np.isfinite(kl_row).all() and np.isfinite(kl) and flag == 0
    worst_dy, worst_kl = np.abs(dy - want_dy).max(), abs(kl - want_kl.mean())
    print("N = %d, V = %d, tau = %g, alpha = %g: worst dy deviation %.2e (bar %.2e), kl %.8f against %.8f (deviation %.2e)" % (
        N, V, tau, alpha, worst_dy, 2e-5 * s * (1 + alpha * tau), kl, want_kl.mean(), worst_kl))
    assert worst_dy <= 2e-5 * s * (1 + alpha * tau)
    assert np.array_equal(tgt, ys[np.arange(N), target])
    assert worst_kl <= 1e-5
    if V > 1:
        assert want_kl.mean() > 0.1                                    # two unrelated distributions: the kl is there to be checked
        # one window of all the words: the same kl_row bits, since the windows start on multiples of 64
        _dy1, tgt1, kl_row1, kl1, _f = _pass2(ys, yt, [(0, V)], tau, alpha, target, nw)
        assert np.array_equal(kl_row1, kl_row) and kl1 == kl and np.array_equal(tgt1, tgt)


def test_kl_mean_flags_what_is_not_finite():
    O = jops.backend()
    for bad in (float("nan"), float("inf")):
        kl_row = torch.full((37,), 0.25, device="cuda")
        kl_row[36] = bad
        kl, flag = _nan(2, dtype=torch.float64), torch.zeros(1, device="cuda", dtype=torch.int32)
        O.train_distill_kl(kl_row, 37, kl, flag)
        assert float(kl[0]) == float("inf") and int(flag[0]) == 1
    kl_row = torch.full((300,), 0.25, device="cuda")
    kl, flag = _nan(2, dtype=torch.float64), torch.zeros(1, device="cuda", dtype=torch.int32)
    O.train_distill_kl(kl_row, 300, kl, flag)
    assert float(kl[0]) == 0.25 and int(flag[0]) == 0


# ---- one step
def _student(mode, V=2000, H=64, E=32, segs=None):
    cfg = synth.make_config(V, H, E, mode, segs or synth.small_segs(V), True)
    return cfg, T.init_weights(cfg, None, 101)


def _teacher(kind, V=2000):
    if kind == "vtable":                                               # other H, E and cuts than the student's
        cfg = synth.make_config(V, 96, 48, "vtable", [(48, 0, (7 * V) // 20), (24, (7 * V) // 20, None)], True)
    elif kind == "tied":
        cfg = synth.make_config(V, 48, 40, "tied", synth.small_segs(V), False)
    else:
        cfg = synth.make_config(V, 31, 17, "tied", synth.small_segs(V), False)
    w = T.init_weights(cfg, None, 23)
    return cfg, {k: (a * 3.0).astype(np.float32) for k, a in w.items()}                # logits of some spread: a kl worth the name


def _pair(cfg, w, tcfg, tw, B, Tn, chunk_bytes=None, **kw):
    kw = dict(dict(lr=1e-3, dropout=0.9, norm_weight=0.1, seed=42, alpha=0.5, temperature=2.5), **kw)
    return (D.DistillReferenceStepper(cfg, w, tcfg, tw, B, Tn, **kw),
            D.DistillDeviceStepper(cfg, w, tcfg, tw, B, Tn, chunk_bytes=chunk_bytes, **kw))


def _compare_step(cfg, w, tcfg, tw, B, Tn, chunk_bytes, windows, seed=3):
    V, H, Ht = cfg["vocab_size"], cfg["hidden_size"], tcfg["hidden_size"]
    x, y = tc.batch(V, B, Tn, seed)
    ref, dev = _pair(cfg, w, tcfg, tw, B, Tn, chunk_bytes)
    assert [n for _v0, n, _p in dev._windows()] == windows
    for st in (ref, dev):                                              # carried states for both models
        st.set_state(*tc.carried_state(B, H, seed + 1))
        st.set_teacher_state(*tc.carried_state(B, Ht, seed + 2))
    ce_ref, ce_dev = ref.step(x, y), dev.step(x, y)
    kl_ref, kl_dev = ref.kls()[-1], dev.kls()[-1]
    worst = tc.worst_relative(dev.grads(), ref.grads())
    print("ce %.6f / %.6f, kl %.6f / %.6f; worst relative gradient deviation per tensor: %s" % (
        ce_dev, ce_ref, kl_dev, kl_ref, {k: "%.2e" % v for k, v in worst.items()}))
    assert abs(ce_ref - ce_dev) <= 1e-5 and abs(kl_ref - kl_dev) <= 1e-5 and kl_ref > 1e-3
    for k, v in worst.items():
        assert v <= 1e-4, (k, v)
    # both carried states are the restatement's
    np.testing.assert_allclose(dev.tHs[:B].cpu().numpy(), ref.th, rtol=0, atol=1e-5)
    np.testing.assert_allclose(dev.Hs[:B].cpu().numpy(), ref.h, rtol=0, atol=1e-5)


@pytest.mark.parametrize("mode", ["tied", "vtable", "dsoftmax"])
@pytest.mark.parametrize("teacher", ["vtable", "tied"])
def test_step_gradients(mode, teacher):
    cfg, w = _student(mode)
    tcfg, tw = _teacher(teacher)
    _compare_step(cfg, w, tcfg, tw, 32, 10, 2 * 4 * 320 * 768, [768, 768, 464])       # half the budget each: three windows
    _compare_step(cfg, w, tcfg, tw, 13, 7, None, [2000])                                # one window, rows no multiple of a tile


@pytest.mark.parametrize("mode", ["tied", "vtable", "dsoftmax"])
@pytest.mark.parametrize("B,Tn", [(7, 5), (1, 1)])
def test_step_gradients_odd_sizes(mode, B, Tn):
    cfg = tc.odd_cfg(mode)
    w = T.init_weights(cfg, None, 101)
    tcfg, tw = _teacher("odd", tc.ODD_V)
    _compare_step(cfg, w, tcfg, tw, B, Tn, 2 * 4 * B * Tn * 64, [64, 64, 29])


# ---- the degenerate form, the frozen teacher
@pytest.mark.parametrize("mode", ["tied", "vtable", "dsoftmax"])
def test_alpha_zero_enqueues_the_plain_step(mode):
    cfg, w = _student(mode)
    tcfg, tw = _teacher("vtable")
    kw = dict(lr=1e-3, dropout=0.9, norm_weight=0.1, seed=7, chunk_bytes=4 * 320 * 768)
    plain = T.DeviceStepper(cfg, w, 32, 10, **kw)
    st = D.DistillDeviceStepper(cfg, w, tcfg, tw, 32, 10, alpha=0.0, temperature=2.5, **kw)
    assert st.Vc == plain.Vc and not hasattr(st, "Yt")                 # no teacher on the device at all
    for i in range(3):
        x, y = tc.batch(2000, 32, 10, 60 + i)
        plain.step_async(x, y)
        st.step_async(x, y)
    assert np.array_equal(plain.losses(), st.losses()) and len(st.kls()) == 0
    assert torch.equal(plain.W, st.W) and torch.equal(plain.M, st.M) and torch.equal(plain.Vv, st.Vv)


def test_teacher_buffers_never_change():
    cfg, w = _student("tied")
    tcfg, tw = _teacher("vtable")
    _ref, dev = _pair(cfg, w, tcfg, tw, 32, 10, 2 * 4 * 320 * 768)
    before = {k: v.clone() for k, v in dev.teacher_buffers().items()}
    assert {("LM0", None), ("LM1", None), ("VT1", None), ("PM", None), ("b2", None), ("HM", None), ("IM", None), ("b", None),
            ("Emb", None)} == set(before)
    w0 = dev.W.clone()
    for i in range(5):
        dev.step_async(*tc.batch(2000, 32, 10, 70 + i))
    dev.losses()
    assert not torch.equal(dev.W, w0)
    for k, v in dev.teacher_buffers().items():
        assert torch.equal(v, before[k]), k
    got, emb = before[("Emb", None)].cpu().numpy(), T.build_embedding(tw, dev.td)      # the Emb assembled once is the teacher's
    cut = dev.td["segs"][0][2]
    assert np.array_equal(got[:cut], tw["LM0"])
    bound = 1.01 * (24 + 2) * U * (np.abs(tw["LM1"]).astype(np.float64) @ np.abs(tw["VT1"]).astype(np.float64))     # a 24-term f32 chain
    assert np.all(np.abs(got[cut:] - emb[cut:]) <= bound)


# ---- twenty steps, the chunk budget
@pytest.mark.parametrize("mode,teacher,lr", [("tied", "vtable", 1e-3), ("vtable", "tied", 5e-3), ("dsoftmax", "vtable", 1e-3)])
def test_twenty_steps(mode, teacher, lr):
    cfg, w = _student(mode)
    tcfg, tw = _teacher(teacher)
    ref, dev = _pair(cfg, w, tcfg, tw, 32, 10, lr=lr, seed=7, alpha=0.5, temperature=2.0)
    for i in range(20):
        x, y = tc.batch(2000, 32, 10, 100 + i)
        ref.step_async(x, y)
        dev.step_async(x, y)
    d_ce, d_kl = np.abs(ref.losses() - dev.losses()).max(), np.abs(ref.kls() - dev.kls()).max()
    print("largest |ce_dev - ce_ref| %.2e, |kl_dev - kl_ref| %.2e over 20 steps" % (d_ce, d_kl))
    assert len(dev.kls()) == 20 and d_ce <= 1e-5 and d_kl <= 1e-5
    wr, wd = dict(tc.flat_items(ref.weights())), dict(tc.flat_items(dev.weights()))
    drift = {k: float(np.abs(wr[k].astype(np.float64) - wd[k]).max()) for k in wr}
    print("weight drift after 20 steps in units of lr:", {k: "%.2e" % (v / lr) for k, v in drift.items()})
    for k, v in drift.items():
        assert v <= 20 * lr * 1e-3, (k, v)


@pytest.mark.parametrize("mode", ["tied", "vtable"])
def test_chunk_budget_leaves_ce_and_kl_the_same_bits(mode):
    cfg, w = _student(mode)
    tcfg, tw = _teacher("vtable")
    _r, one = _pair(cfg, w, tcfg, tw, 32, 10, None)
    _r, three = _pair(cfg, w, tcfg, tw, 32, 10, 2 * 4 * 320 * 768)
    assert len(one._windows()) == 1 and len(three._windows()) == 3
    x, y = tc.batch(2000, 32, 10, 500)
    one.step_async(x, y)
    three.step_async(x, y)
    assert one.losses()[0] == three.losses()[0] and one.kls()[0] == three.kls()[0]
    assert torch.equal(one.kl_row, three.kl_row) and torch.equal(one.run, three.run)


# ---- the driver
@pytest.fixture(scope="module")
def corpus_root():
    root = tempfile.mkdtemp(prefix="jlm_distill_gpu_")
    streams = tc.write_markov_corpus(root, n_train=2032, n_dev=432, n_test=432)
    teacher = T.train_experiment(tc.driver_parameters("vtable", self_norm=True, max_epochs=1), root=root, log=lambda s: None)
    return root, streams, teacher


STUDENT = dict(hidden_size=32, max_epochs=2)


def _disk_weights(exp):
    with open(os.path.join(jconfig.experiment_path, str(exp), "weights", "lstm_weights.pkl"), "rb") as f:
        return pickle.load(f)


def test_two_runs_write_the_same_bytes(corpus_root):
    root, _streams, teacher = corpus_root
    p = tc.driver_parameters("tied", self_norm=True, **STUDENT)
    a, b = (_disk_weights(D.distill_experiment(teacher, p, alpha=0.5, temperature=2.0, root=root, log=lambda s: None)) for _ in range(2))
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


def test_distill_then_score_and_decode(corpus_root):
    from jlm_amd import perplexity
    from jlm_amd.decoder import Decoder
    from jlm_amd.model import LSTM_Model
    root, (_train, _dev, test), teacher = corpus_root
    p = tc.driver_parameters("tied", **STUDENT)
    exp = D.distill_experiment(teacher, p, alpha=0.5, temperature=2.0, root=root, log=lambda s: None)
    got = dict(D.last_result)
    D.distill_experiment(teacher, p, alpha=0.5, temperature=2.0, root=root, log=lambda s: None, stepper="reference")
    want = dict(D.last_result)
    print("validation perplexities: device %s, restatement %s" % ([v for _t, v in got["history"]], [v for _t, v in want["history"]]))
    assert len(got["history"]) == 2
    assert abs(got["best_valid_pp"] - want["best_valid_pp"]) <= 1e-4 * want["best_valid_pp"]
    jconfig.set_root(root)
    pp, _total, _n = perplexity.stream_perplexity(LSTM_Model(exp), test, p["batch_size"], p["num_steps"])
    print("test perplexity: trainer %.6f, scoring path %.6f" % (got["best_test_pp"], pp))
    assert abs(pp - got["best_test_pp"]) <= 2e-5 * got["best_test_pp"]
    outs = Decoder(exp).decode_batch(synth.make_ragged_sentences(3, 3, 8, seed=42, alphabet=12), beam_width=5)
    assert len(outs) == 3


# ---- the non-finite path
def test_an_infinite_teacher_stops_the_run():
    """one infinite entry in the teacher's PM: its logits, A_t and the kl are not numbers while the student's ce is finite.  Nothing
    faults: the step runs to its end, the kl kernel raises the flag word, Adam does not touch the student's weights."""
    cfg, w = _student("tied")
    tcfg, tw = _teacher("tied")
    tw["PM"][3, 5] = np.inf
    _ref, dev = _pair(cfg, w, tcfg, tw, 32, 10)
    x, y = tc.batch(2000, 32, 10, 5)
    dev.step_async(x, y, train=False)                                  # an evaluation step does not meet the teacher
    assert np.isfinite(dev.losses()).all()
    dev.step_async(x, y)
    with pytest.raises(T.NonFiniteLoss) as e:
        dev.losses()
    assert e.value.step == 1
    assert np.isfinite(dev.ce[:2].cpu().numpy()).all() and float(dev.kl[0]) == float("inf")
    after = dev.weights()
    assert all(np.array_equal(after[k], w[k]) for k in w)
    torch.cuda.synchronize()
