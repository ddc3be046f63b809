"""GPU: training on the device (jlm_amd.train.DeviceStepper over csrc/jlm_train.hip through torch.ops.jlm.train_*) against the numpy
float64 restatement (ReferenceStepper): every kernel as launched, one step's gradients, twenty steps, reproducibility, the whole driver
on the Markov corpus with the trained experiment scored and decoded by the inference side, and the non-finite path.

The kernel bars are worst-case rounding bounds of an f32 chain (u = 2^-24: a K-term fmaf chain errs by at most K u sum|a b|); the step,
twenty-step and end-to-end bars are the project's own (1e-4 relative per gradient tensor, 1e-5 per-token ce, 20 lr 1e-3 weight drift,
1e-4 / 2e-5 relative perplexity)."""
import os
import pickle
import tempfile

import numpy as np
import pytest

torch = pytest.importorskip("torch")
from jlm_amd import config as jconfig, ops as jops, synth, train as T      # noqa: E402
from tests import train_cases as tc                                        # noqa: E402

pytestmark = pytest.mark.gpu
U = 2.0 ** -24


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype=dtype)


def _signed(k):
    return T._signed64(k)


# ---- 7. the kernels, as launched
GEMM_SHAPES = [(1, 1, 1), (37, 70, 1), (65, 130, 37), (100, 257, 2560), (130, 33, 2560), (64, 64, 16), (3, 2049, 200), (2560, 50, 37)]


@pytest.mark.parametrize("form", ["nt", "tn", "nn"])
@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
def test_gemm_forms(form, M, N, K):
    rng = np.random.RandomState(M + 7 * N + 13 * K)
    a = rng.normal(size=(M, K)).astype(np.float32)
    b = rng.normal(size=(K, N)).astype(np.float32)
    bias = rng.normal(size=N).astype(np.float32)
    c0 = rng.normal(size=(M, N + 3)).astype(np.float32)
    O = jops.backend()
    if form == "nt":        # both K-contiguous: A [M, K], B stored [N, K]
        A, sam, sak, B, sbk, sbn = _dev(a), K, 1, _dev(b.T.copy()), 1, K
    elif form == "tn":      # contracts over rows: A stored [K, M], B [K, N]
        A, sam, sak, B, sbk, sbn = _dev(a.T.copy()), 1, M, _dev(b), N, 1
    else:
        A, sam, sak, B, sbk, sbn = _dev(a), K, 1, _dev(b), N, 1
    exact = a.astype(np.float64) @ b.astype(np.float64)
    bound = 1.01 * (K + 2) * U * (np.abs(a).astype(np.float64) @ np.abs(b).astype(np.float64) + np.abs(bias) + np.abs(c0[:, :N]))
    C = _dev(c0)
    O.train_gemm(A, sam, sak, B, sbk, sbn, C, N + 3, M, N, K, False, None)
    got = C.cpu().numpy()
    assert np.all(np.abs(got[:, :N] - exact) <= bound), (form, M, N, K, np.abs(got[:, :N] - exact).max())
    assert np.array_equal(got[:, N:], c0[:, N:])              # the columns past N are not touched
    C = _dev(c0)
    O.train_gemm(A, sam, sak, B, sbk, sbn, C, N + 3, M, N, K, True, _dev(bias))
    got2 = C.cpu().numpy()
    assert np.all(np.abs(got2[:, :N] - (exact + bias + c0[:, :N])) <= bound), (form, M, N, K)
    assert np.array_equal(got2[:, N:], c0[:, N:])
    C = _dev(c0)
    O.train_gemm(A, sam, sak, B, sbk, sbn, C, N + 3, M, N, K, False, None)
    assert np.array_equal(C.cpu().numpy(), got)               # the same bits, run after run


@pytest.mark.parametrize("keep", [1.0, 0.9])
def test_embed_rows_and_mask(keep):
    rng = np.random.RandomState(1)
    V, E, n = 300, 37, 91
    emb = rng.normal(size=(V, E)).astype(np.float32)
    ids = rng.randint(0, V, n).astype(np.int32)
    x = torch.zeros(n, E, device="cuda")
    key = T.mask_key(5, 3, 0)
    jops.backend().train_embed_rows(_dev(emb), E, V, _dev(ids), n, E, x, _signed(key), T.keep_threshold(keep), 1.0 / keep)
    mask = T.dropout_mask(5, 3, 0, (n, E), keep)
    want = np.where(mask != 0, emb[ids] * np.float32(1.0 / keep), np.float32(0))
    assert np.array_equal(x.cpu().numpy(), want)


@pytest.mark.parametrize("B,H", [(1, 1), (7, 24), (37, 64), (128, 512)])
def test_cell_forward_backward(B, H):
    rng = np.random.RandomState(B + H)
    z = rng.normal(0, 1.5, (B, 4 * H)).astype(np.float32)
    c_prev = rng.normal(size=(B, H)).astype(np.float32)
    keep, row0 = 0.9, 3 * B
    key = T.mask_key(11, 2, 1)
    thr, scale = T.keep_threshold(keep), 1.0 / keep
    mask = T.dropout_mask(11, 2, 1, (B, H), keep, offset=row0 * H)
    O = jops.backend()
    zd, c, h, r = _dev(z), torch.zeros(B, H, device="cuda"), torch.zeros(B, H, device="cuda"), torch.zeros(B, H, device="cuda")
    O.train_cell_fwd(zd, _dev(c_prev), c, h, r, B, H, row0, _signed(key), thr, scale)
    z64 = z.astype(np.float64)
    sg = lambda v: 1.0 / (1.0 + np.exp(-v))
    gi, gf, go, gg = sg(z64[:, :H]), sg(z64[:, H:2 * H]), sg(z64[:, 2 * H:3 * H]), np.tanh(z64[:, 3 * H:])
    c64 = c_prev * gf + gg * gi
    h64 = np.tanh(c64) * go
    tol = lambda ref: 32 * U * max(1.0, np.abs(ref).max())
    gates = zd.cpu().numpy()
    np.testing.assert_allclose(gates, np.concatenate([gi, gf, go, gg], axis=1), rtol=0, atol=tol(gg))
    np.testing.assert_allclose(c.cpu().numpy(), c64, rtol=0, atol=tol(c64))
    np.testing.assert_allclose(h.cpu().numpy(), h64, rtol=0, atol=tol(h64))
    np.testing.assert_allclose(r.cpu().numpy(), h64 * mask, rtol=0, atol=tol(h64 * mask))
    assert np.array_equal(r.cpu().numpy() == 0, (mask == 0) | (h.cpu().numpy() == 0))
    # backward, on the gates the forward kernel left
    dr = rng.normal(size=(B, H)).astype(np.float32)
    dh_next = rng.normal(size=(B, H)).astype(np.float32)
    dc_in = rng.normal(size=(B, H)).astype(np.float32)
    g64 = gates.astype(np.float64)
    gi, gf, go, gg = g64[:, :H], g64[:, H:2 * H], g64[:, 2 * H:3 * H], g64[:, 3 * H:]
    c32 = c.cpu().numpy().astype(np.float64)
    for nxt in (dh_next, None):
        dc, dz = _dev(dc_in), torch.zeros(B, 4 * H, device="cuda")
        O.train_cell_bwd(zd, c, _dev(c_prev), _dev(dr), None if nxt is None else _dev(nxt), dc, dz, B, H, row0, _signed(key), thr, scale)
        dh = dr * mask + (0 if nxt is None else nxt)
        tcn = np.tanh(c32)
        dcc = dc_in + dh * go * (1 - tcn * tcn)
        want = np.concatenate([dcc * gg * gi * (1 - gi), dcc * c_prev * gf * (1 - gf), dh * tcn * go * (1 - go), dcc * gi * (1 - gg * gg)], axis=1)
        np.testing.assert_allclose(dz.cpu().numpy(), want, rtol=0, atol=tol(want))
        np.testing.assert_allclose(dc.cpu().numpy(), dcc * gf, rtol=0, atol=tol(dcc))


@pytest.mark.parametrize("norm_weight", [0.0, 0.1])
def test_loss_kernels_over_chunks(norm_weight):
    """the normaliser over chunks, dy in place, the target's logit (targets in the first and the last chunk), db2 and ce"""
    rng = np.random.RandomState(4)
    N, V, Vc = 37, 1000, 384                                   # chunks of 384, 384, 232 words
    y = rng.normal(0, 2.0, (N, V)).astype(np.float32)
    target = rng.randint(0, V, N).astype(np.int32)
    target[:4] = [0, 383, V - 1, 768]
    O = jops.backend()
    run_m, run_s, tgt = (torch.zeros(N, device="cuda") for _ in range(3))
    Y = torch.zeros(N, Vc, device="cuda")
    yd, td = _dev(y), _dev(target)
    chunks = [(v0, min(Vc, V - v0)) for v0 in range(0, V, Vc)]
    for k, (v0, n) in enumerate(chunks):
        Y[:, :n].copy_(yd[:, v0:v0 + n])
        O.train_lse_update(Y, Vc, n, N, run_m, run_s, k == 0)
    y64 = y.astype(np.float64)
    lse = np.log(np.exp(y64 - y64.max(1, keepdims=True)).sum(1)) + y64.max(1)
    got_lse = (run_m + torch.log(run_s)).cpu().numpy()
    np.testing.assert_allclose(got_lse, lse, rtol=0, atol=4 * U * 16)           # four ulp of a value below 16
    s, nw2 = 1.0 / N, 2.0 * norm_weight
    want = np.exp(y64 - lse[:, None]) * (1 + nw2 * lse)[:, None]
    want[np.arange(N), target] -= 1
    want *= s
    db2 = torch.zeros(V, device="cuda")
    for v0, n in chunks:
        Y[:, :n].copy_(yd[:, v0:v0 + n])
        O.train_dy(Y, Vc, n, v0, N, run_m, run_s, td, tgt, s, nw2)
        np.testing.assert_allclose(Y[:, :n].cpu().numpy(), want[:, v0:v0 + n], rtol=0, atol=2e-5 * s)
        O.train_colsum(Y, Vc, N, n, db2[v0:v0 + n], False)
    assert np.array_equal(tgt.cpu().numpy(), y[np.arange(N), target])
    np.testing.assert_allclose(db2.cpu().numpy(), want.sum(0), rtol=0, atol=N * 2e-5 * s + N * U * np.abs(want).sum(0).max())
    ce, flag = torch.zeros(2, device="cuda", dtype=torch.float64), torch.zeros(1, device="cuda", dtype=torch.int32)
    O.train_ce(run_m, run_s, tgt, N, norm_weight, ce, flag)
    assert abs(float(ce[0]) - float(np.mean(lse - y64[np.arange(N), target]))) <= 4 * U * 16 and int(flag[0]) == 0
    O.train_colsum(Y, Vc, N, chunks[-1][1], db2[:chunks[-1][1]], True)          # accumulate on top
    assert torch.isfinite(db2).all()


@pytest.mark.parametrize("case", ["one word", "mixed", "distinct"])
@pytest.mark.parametrize("part", ["all", "block"])
def test_sorted_scatter(case, part):
    """all: every word and column; block: the words [v_lo, v_hi) and columns [col0, col0 + n_cols) only (a D_softmax block)"""
    rng = np.random.RandomState(8)
    n, E, V = 2560 if case == "one word" else 300, 37, 400 if case == "distinct" else 50
    ids = {"one word": np.full(n, 17), "mixed": rng.randint(0, 30, n), "distinct": rng.permutation(V)[:n]}[case]
    ids = ids.astype(np.int32)
    v_lo, v_hi, col0, nc = (0, V, 0, E) if part == "all" else (11, V - 5, 6, 19)
    dx = rng.normal(size=(n, E)).astype(np.float32)
    base = rng.normal(size=(v_hi - v_lo, nc + 2)).astype(np.float32)
    keep = 0.9
    key = T.mask_key(3, 9, 0)
    mask = T.dropout_mask(3, 9, 0, (n, E), keep)
    srt, perm = torch.sort(_dev(ids), stable=True)
    outs = []
    for _ in range(2):
        demb = _dev(base)
        jops.backend().train_scatter_rows(_dev(dx), E, col0, nc, E, srt, perm, n, demb, nc + 2, v_lo, v_hi, _signed(key),
                                          T.keep_threshold(keep), 1.0 / keep)
        outs.append(demb.cpu().numpy())
    assert np.array_equal(outs[0], outs[1])
    assert np.array_equal(outs[0][:, nc:], base[:, nc:])                       # the columns past the block are not touched
    want = base[:, :nc].astype(np.float64)
    mag = np.abs(want)
    inside = (ids >= v_lo) & (ids < v_hi)
    np.add.at(want, ids[inside] - v_lo, (dx * mask)[inside][:, col0:col0 + nc])
    np.add.at(mag, ids[inside] - v_lo, np.abs(dx * mask)[inside][:, col0:col0 + nc])
    count = np.bincount(ids, minlength=V).max()
    assert np.all(np.abs(outs[0][:, :nc] - want) <= 1.01 * (count + 2) * U * mag + 1e-30)


def test_adam_kernel():
    rng = np.random.RandomState(2)
    n, lr = 4 * 1031, 5e-3
    w = rng.normal(size=n).astype(np.float32)
    m, v = np.zeros(n), np.zeros(n)
    w64 = w.astype(np.float64)
    wd, md, vd = _dev(w), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    flag = torch.zeros(1, device="cuda", dtype=torch.int32)
    for t in range(1, 6):
        g = (rng.normal(size=n) * 10.0 ** rng.uniform(-6, 0, n)).astype(np.float32)
        w64, m, v = T.adam_reference(w64, g.astype(np.float64), m, v, t, lr)
        jops.backend().train_adam(wd, _dev(g), md, vd, n, T.adam_lr_t(lr, t), flag)
        # a step moves an element by at most ~lr_t; eight ulp of that and one of the weight per step
        np.testing.assert_allclose(wd.cpu().numpy(), w64, rtol=0, atol=t * (8 * U * 3 * lr + U * np.abs(w64).max()))
    before = wd.clone()
    flag.fill_(1)
    jops.backend().train_adam(wd, _dev(g), md, vd, n, T.adam_lr_t(lr, 6), flag)
    assert torch.equal(wd, before)                                              # a raised flag stops every update


# ---- 8. one step's gradients
def _fixture(mode, self_norm, V=2000, H=64, E=32, segs=None):
    cfg = synth.make_config(V, H, E, mode, segs or synth.small_segs(V), self_norm)
    return cfg, T.init_weights(cfg, None, 101)


def _batch(V, B, Tn, seed):
    rng = np.random.RandomState(seed)
    return rng.randint(0, V, (B, Tn)), rng.randint(0, V, (B, Tn))


def _compare_grads(cfg, w, B, Tn, chunk_bytes=None, state=True, seed=3):
    V, H = cfg["vocab_size"], cfg["hidden_size"]
    x, y = _batch(V, B, Tn, seed)
    kw = dict(lr=1e-3, dropout=0.9, norm_weight=0.1, seed=42)
    ref = T.ReferenceStepper(cfg, w, B, Tn, **kw)
    dev = T.DeviceStepper(cfg, w, B, Tn, chunk_bytes=chunk_bytes, **kw)
    if state:
        rng = np.random.RandomState(seed + 1)
        h0, c0 = rng.normal(0, 0.3, (B, H)).astype(np.float32), rng.normal(0, 0.3, (B, H)).astype(np.float32)
        ref.set_state(h0, c0)
        dev.set_state(h0, c0)
    ce_ref, ce_dev = ref.step(x, y), dev.step(x, y)
    assert abs(ce_ref - ce_dev) <= 1e-5, (ce_ref, ce_dev)
    want, got = dict(tc.flat_items(ref.grads())), dict(tc.flat_items(dev.grads()))
    assert sorted(want) == sorted(got)
    worst = {}
    for k in want:
        worst[k] = np.abs(got[k] - want[k]).max() / np.abs(want[k]).max()
    print("ce %.6f / %.6f; worst relative gradient deviation per tensor: %s" % (ce_dev, ce_ref, {k: "%.2e" % v for k, v in worst.items()}))
    for k, v in worst.items():
        assert v <= 1e-4, (k, v)
    return dev, ref


@pytest.mark.parametrize("mode", ["tied", "vtable", "dsoftmax"])
@pytest.mark.parametrize("self_norm", [False, True])
def test_step_gradients_small(mode, self_norm):
    cfg, w = _fixture(mode, self_norm)
    N = 32 * 10
    _compare_grads(cfg, w, 32, 10, chunk_bytes=4 * N * 768)              # three chunks of words: 768, 768, 464
    _compare_grads(cfg, w, 13, 7, state=False)                           # one chunk, rows no multiple of a tile


def test_step_gradients_mid_vtable():
    """the headline sizes: V = 50 000, H = 512, segments 200 / 100 / 50, B = 128, T = 20 (two chunks of words at the default budget)"""
    cfg, w = _fixture("vtable", True, 50000, 512, 256, synth.README_SEGS)
    _compare_grads(cfg, w, 128, 20)


# ---- 9. twenty steps
@pytest.mark.parametrize("mode,self_norm,lr", [("tied", False, 1e-3), ("vtable", True, 5e-3), ("dsoftmax", True, 1e-3)])
def test_twenty_steps(mode, self_norm, lr):
    cfg, w = _fixture(mode, self_norm)
    B, Tn, V = 32, 10, cfg["vocab_size"]
    kw = dict(lr=lr, dropout=0.9, norm_weight=0.1, seed=7)
    ref, dev = T.ReferenceStepper(cfg, w, B, Tn, **kw), T.DeviceStepper(cfg, w, B, Tn, **kw)
    for i in range(20):
        x, y = _batch(V, B, Tn, 100 + i)
        ref.step_async(x, y)
        dev.step_async(x, y)
    a, b = ref.losses(), dev.losses()
    print("largest |ce_dev - ce_ref| over 20 steps: %.2e" % np.abs(a - b).max())
    assert np.abs(a - b).max() <= 1e-5
    wr, wd = dict(tc.flat_items(ref.weights())), dict(tc.flat_items(dev.weights()))
    drift = {k: float(np.abs(wr[k].astype(np.float64) - wd[k]).max()) for k in wr}
    print("weight drift after 20 steps in units of lr:", {k: "%.2e" % (v / lr) for k, v in drift.items()})
    for k, v in drift.items():
        assert v <= 20 * lr * 1e-3, (k, v)


# ---- 10. reproducibility
@pytest.fixture(scope="module")
def corpus_root():
    root = tempfile.mkdtemp(prefix="jlm_train_gpu_")
    return root, tc.write_markov_corpus(root)


def _disk_weights(exp):
    with open(os.path.join(jconfig.experiment_path, str(exp), "weights", "lstm_weights.pkl"), "rb") as f:
        return pickle.load(f)


def test_two_runs_write_the_same_bytes(corpus_root):
    root, _ = corpus_root
    p = tc.driver_parameters("vtable", self_norm=True, max_epochs=1)
    a = _disk_weights(T.train_experiment(p, root=root, log=lambda s: None))
    b = _disk_weights(T.train_experiment(p, root=root, log=lambda s: None))
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


def test_chunk_budget_changes_the_sums_not_the_loss():
    cfg, w = _fixture("tied", True)
    B, Tn, V = 32, 10, cfg["vocab_size"]
    kw = dict(lr=1e-3, dropout=0.9, norm_weight=0.1, seed=7)
    budget = 4 * B * Tn * 1024
    one, half = T.DeviceStepper(cfg, w, B, Tn, chunk_bytes=budget, **kw), T.DeviceStepper(cfg, w, B, Tn, chunk_bytes=budget // 2, **kw)
    assert (one.Vc, half.Vc) == (1024, 512)
    for i in range(20):
        x, y = _batch(V, B, Tn, 500 + i)
        one.step_async(x, y)
        half.step_async(x, y)
    assert np.abs(one.losses() - half.losses()).max() <= 1e-5


# ---- 11. end to end
@pytest.mark.parametrize("mode", ["tied", "vtable"])
def test_train_then_score_and_decode(corpus_root, mode):
    from jlm_amd import perplexity
    from jlm_amd.decoder import Decoder
    from jlm_amd.model import LSTM_Model
    from oracle import jlm_oracle as orc
    from tests.test_gpu_decode import _check_nbest
    root, (train, dev, test) = corpus_root
    uni = tc.unigram_perplexity(train, dev)
    p = tc.driver_parameters(mode)
    exp = T.train_experiment(p, root=root, log=lambda s: None)
    got = dict(T.last_result)
    T.train_experiment(p, root=root, log=lambda s: None, stepper="reference")
    want = dict(T.last_result)
    print("validation perplexities: device %s, restatement %s (unigram %.1f)" % ([v for _t, v in got["history"]],
                                                                                [v for _t, v in want["history"]], uni))
    assert got["best_valid_pp"] < uni / 4
    assert abs(got["best_valid_pp"] - want["best_valid_pp"]) <= 1e-4 * want["best_valid_pp"]
    jconfig.set_root(root)
    model = LSTM_Model(exp)
    pp, _total, _n = perplexity.stream_perplexity(model, test, p["batch_size"], p["num_steps"])
    print("test perplexity: trainer %.6f, scoring path %.6f" % (got["best_test_pp"], pp))
    assert abs(pp - got["best_test_pp"]) <= 2e-5 * got["best_test_pp"]
    sents = synth.make_ragged_sentences(5, 3, 10, seed=42, alphabet=12)
    outs = Decoder(exp).decode_batch(sents, beam_width=5)
    oracle = orc.OracleDecoder(root, exp)
    for s, out in zip(sents, outs):
        _check_nbest(out, oracle.decode(s, beam_width=5), (mode, s), len(s))


# ---- 12. the non-finite path
def test_non_finite_loss_stops_the_run(corpus_root):
    """one 1e30 entry in PM: the logits reach 1e29, their log-normaliser squared -- the self-normalisation term of the loss -- is inf
    in float32.  Nothing faults: the step runs to its end, the flag word is raised, Adam does not touch the weights."""
    root, _ = corpus_root
    p = tc.driver_parameters("tied", self_norm=True, max_epochs=1)
    w = T.init_weights(p, 600, 101)
    w["PM"][3, 5] = 1e30
    made = {}

    def factory(cfg, weights, **kw):
        made["st"] = T.DeviceStepper(cfg, weights, **kw)
        return made["st"]
    with pytest.raises(T.NonFiniteLoss) as e:
        T.train_experiment(p, root=root, log=lambda s: None, stepper=factory, initial_weights=w)
    assert e.value.epoch == 0 and e.value.step == 0
    after = made["st"].weights()
    assert all(np.array_equal(after[k], w[k]) for k in w)
    torch.cuda.synchronize()
