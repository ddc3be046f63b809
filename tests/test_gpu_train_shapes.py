"""GPU: the device training step (jlm_amd.train.DeviceStepper, jlm_amd.finetune.CodebookDeviceStepper over csrc/jlm_train.hip) at the
shapes tests/test_gpu_train.py leaves out: a model none of whose sizes is a multiple of 4 (V = 157, H = 23, widths 19 / 9 / 5, so the
flat parameter buffer has padding between its tensors), T = 1 and B = 1, the evaluation pass step by step, more than 256 steps without
a read-back, and ``train_gemm`` with the strided views ``step_async`` hands it.

Everything is judged against the float64 restatement (ReferenceStepper / CodebookReferenceStepper, themselves pinned to autograd at
these sizes by tests/test_train_cpu.py) on the bars of tests/test_gpu_train.py: ce within 1e-5, every gradient tensor within 1e-4 of its
largest reference magnitude, a weight within lr 1e-3 per step; the carried state within 32 u, u = 2^-24 (the bar of
``test_cell_forward_backward``; |h|, |c| stay below 1 here).  Float32 autograd of the same graph sits at most 1.0e-6 (gradients) and 6.9e-7
(ce) from the restatement over the thirty step cases below, so the bars have room."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
from jlm_amd import finetune as F, ops as jops, train as T                  # noqa: E402
from tests import train_cases as tc                                        # noqa: E402

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
NAN = float("nan")
V, H, H4 = tc.ODD_V, tc.ODD_H, 4 * tc.ODD_H
E, ED = 19, 33                       # the embedding width of the tied / V_table model and of the D_softmax one
NB, NT, NR = 7, 5, 35                # the batch of the GEMM cases: B, T and N = B T rows
ONE_WINDOW, WINDOWS_OF_64 = None, 1  # chunk_bytes: the default budget holds all 157 words; one byte gives the floor Vc = 64


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- 1. train_gemm with the operands the step launches
# An operand is (shape of the buffer the stepper holds, the slice of it the launch passes, the part of that slice the launch may touch
# -- None: all of it).  The buffer sits in a NaN-filled storage with 8 words before and after it, and only the part the launch may touch
# holds numbers: a read outside it poisons the result, a write outside it shows.  The strides are those of the call in
# jlm_amd/train.py; the sizes are the odd model's at B = 7, T = 5: N = 35 rows, segments [0, 40) k = 19, [40, 93) k = 9, [93, 157)
# k = 5, and with Vc = 64 the windows [0, 64), [64, 128), [128, 157), which cut segments 1 and 2.
S = np.s_
LEAD = 8


def _case(name, A, sa, B, sb, C, ldc, M, N, K, acc=False, bias=None):
    return dict(name=name, A=A, sam=sa[0], sak=sa[1], B=B, sbk=sb[0], sbn=sb[1], C=C, ldc=ldc, M=M, N=N, K=K, acc=acc, bias=bias)


GEMM_CASES = [
    # _assemble_embedding
    _case("Emb_i = LM_i VT_i", ((53, 9), S[:], None), (9, 1), ((9, E), S[:], None), (E, 1), ((V, E), S[40:93], None), E, 53, E, 9),
    # the forward pass
    _case("Z = X IM + b", ((NR, E), S[:], None), (E, 1), ((E, H4), S[:], None), (H4, 1), ((NR, H4), S[:], None), H4, NR, H4, E,
          bias=((H4,), S[:])),
    _case("Z_t += h_t-1 HM (rows of Hs and Z)", (((NT + 1) * NB, H), S[21:28], None), (H, 1), ((H, H4), S[:], None), (H4, 1),
          ((NR, H4), S[21:28], None), H4, NB, H4, H, acc=True),
    _case("P = R PM", ((NR, H), S[:], None), (H, 1), ((H, E), S[:], None), (E, 1), ((NR, E), S[:], None), E, NR, E, H),
    _case("Q_i = P VT_i^T", ((NR, E), S[:], None), (E, 1), ((9, E), S[:], None), (1, E), ((NR, 9), S[:], None), 9, NR, 9, E),
    # _logits: a piece (a, n) of the window at v0 writes Y[:, a - v0 : a - v0 + n] and reads b2[a : a + n]
    _case("logits: D_softmax block 2, piece (93, 35) of window 64", ((NR, ED), S[:, 28:33], None), (ED, 1), ((64, 5), S[0:35], None), (1, 5),
          ((NR, 64), S[:, 29:], S[:, 29:64]), 64, NR, 35, 5, bias=((V,), S[93:128])),
    _case("logits: factored segment 1, piece (64, 29) of window 64", ((NR, 9), S[:], None), (9, 1), ((53, 9), S[24:53], None), (1, 9),
          ((NR, 64), S[:, 0:], S[:, 0:29]), 64, NR, 29, 9, bias=((V,), S[64:93])),
    _case("logits: factored segment 1 in the one window", ((NR, 9), S[:], None), (9, 1), ((53, 9), S[:], None), (1, 9),
          ((NR, V), S[:, 40:], S[:, 40:93]), V, NR, 53, 9, bias=((V,), S[40:93])),
    _case("logits: D_softmax block 1 in the one window", ((NR, ED), S[:, 19:28], None), (ED, 1), ((53, 9), S[:], None), (1, 9),
          ((NR, V), S[:, 40:], S[:, 40:93]), V, NR, 53, 9, bias=((V,), S[40:93])),
    _case("logits: tied, all words", ((NR, E), S[:], None), (E, 1), ((V, E), S[:], None), (1, E), ((NR, V), S[:, 0:], None), V, NR, V, E,
          bias=((V,), S[:])),
    _case("logits: tied, piece (128, 29) of window 128", ((NR, E), S[:], None), (E, 1), ((V, E), S[128:157], None), (1, E),
          ((NR, 64), S[:, 0:], S[:, 0:29]), 64, NR, 29, E, bias=((V,), S[128:157])),
    # the second pass over the windows: dy sits where the logits sat
    _case("dBlock = dy^T Q: D_softmax block 2, piece (93, 35)", ((NR, 64), S[:, 29:], S[:, 29:64]), (1, 64), ((NR, ED), S[:, 28:33], None), (ED, 1),
          ((64, 5), S[0:35], None), 5, 35, 5, NR),
    _case("dBlock = dy^T Q: factored segment 1, piece (40, 24)", ((NR, 64), S[:, 40:], S[:, 40:64]), (1, 64), ((NR, 9), S[:], None), (9, 1),
          ((53, 9), S[0:24], None), 9, 24, 9, NR),
    _case("dBlock = dy^T Q: tied, piece (128, 29)", ((NR, 64), S[:, 0:], S[:, 0:29]), (1, 64), ((NR, E), S[:], None), (E, 1),
          ((V, E), S[128:157], None), E, 29, E, NR),
    _case("dBlock = dy^T Q: tied, the one window", ((NR, V), S[:, 0:], None), (1, V), ((NR, E), S[:], None), (E, 1),
          ((V, E), S[:], None), E, V, E, NR),
    _case("dQ = dy Block: columns of dP, a block's first piece", ((NR, 64), S[:, 29:], S[:, 29:64]), (64, 1), ((64, 5), S[0:35], None), (5, 1),
          ((NR, ED), S[:, 28:33], None), ED, NR, 5, 35),
    _case("dQ += dy Block: columns of dP, a later piece", ((NR, 64), S[:, 0:], S[:, 0:29]), (64, 1), ((64, 5), S[35:64], None), (5, 1),
          ((NR, ED), S[:, 28:33], None), ED, NR, 5, 29, acc=True),
    _case("dQ_i = dy LM_i: factored, first piece", ((NR, 64), S[:, 40:], S[:, 40:64]), (64, 1), ((53, 9), S[0:24], None), (9, 1),
          ((NR, 9), S[:], None), 9, NR, 9, 24),
    _case("dQ_i += dy LM_i: factored, later piece", ((NR, 64), S[:, 0:], S[:, 0:29]), (64, 1), ((53, 9), S[24:53], None), (9, 1),
          ((NR, 9), S[:], None), 9, NR, 9, 29, acc=True),
    _case("dP = dy LM: tied, the one window", ((NR, V), S[:, 0:], None), (V, 1), ((V, E), S[:], None), (E, 1), ((NR, E), S[:], None), E, NR, E, V),
    _case("dVT_i = dQ_i^T P", ((NR, 9), S[:], None), (1, 9), ((NR, E), S[:], None), (E, 1), ((9, E), S[:], None), E, 9, E, NR),
    _case("dP += dQ_i VT_i", ((NR, 9), S[:], None), (9, 1), ((9, E), S[:], None), (E, 1), ((NR, E), S[:], None), E, NR, E, 9, acc=True),
    # the backward pass
    _case("dPM = R^T dP", ((NR, H), S[:], None), (1, H), ((NR, E), S[:], None), (E, 1), ((H, E), S[:], None), E, H, E, NR),
    _case("dr = dP PM^T", ((NR, E), S[:], None), (E, 1), ((H, E), S[:], None), (1, E), ((NR, H), S[:], None), H, NR, H, E),
    _case("dh_prev = dz_t HM^T (rows of dZ, HM read transposed)", ((NR, H4), S[21:28], None), (H4, 1), ((H, H4), S[:], None), (1, H4),
          ((NB, H), S[:], None), H, NB, H, H4),
    _case("dHM = h_prev^T dz (the first N of Hs' (T + 1) B rows)", (((NT + 1) * NB, H), S[:], S[0:NR]), (1, H), ((NR, H4), S[:], None), (H4, 1),
          ((H, H4), S[:], None), H4, H, H4, NR),
    _case("dIM = x^T dz", ((NR, E), S[:], None), (1, E), ((NR, H4), S[:], None), (H4, 1), ((E, H4), S[:], None), H4, E, H4, NR),
    _case("dx = dz IM^T", ((NR, H4), S[:], None), (H4, 1), ((E, H4), S[:], None), (1, H4), ((NR, E), S[:], None), E, NR, E, H4),
    # the input side through the factorisation
    _case("dLM_i += D VT_i^T", ((53, E), S[:], None), (E, 1), ((9, E), S[:], None), (1, E), ((53, 9), S[:], None), 9, 53, 9, E, acc=True),
    _case("dVT_i += LM_i^T D", ((53, 9), S[:], None), (1, 9), ((53, E), S[:], None), (E, 1), ((9, E), S[:], None), E, 9, E, 53, acc=True),
]


def _place(rng, shape, view, used=None):
    """-> (the host storage, the device storage, the view the launch gets, bool mask of the storage words the launch may touch)"""
    n = int(np.prod(shape))
    flat = np.full(LEAD + n + 8, NAN, dtype=np.float32)
    mask = np.zeros(flat.shape, dtype=bool)
    used = view if used is None else used
    part = flat[LEAD:LEAD + n].reshape(shape)[used]
    part[...] = rng.normal(size=part.shape)
    mask[LEAD:LEAD + n].reshape(shape)[used] = True
    d = _dev(flat)
    return flat, d, d[LEAD:LEAD + n].view(*shape)[view], mask


def _addressed(flat, mask, off, n0, s0, n1, s1, what):
    """the [n0, n1] array a launch addresses from storage word ``off`` with strides (s0, s1): it must be exactly the part the case
    filled (this pins the case, not the kernel)"""
    idx = off + np.arange(n0)[:, None] * s0 + np.arange(n1)[None, :] * s1
    assert np.array_equal(np.sort(idx.reshape(-1)), np.nonzero(mask)[0]), what
    return idx, flat[idx]


def _rel(stride, extent):
    return "=" if stride == extent else ">" if stride > extent else "<"


def _signature(sam, sak, sbk, sbn, ldc, M, N, K, acc, bias):
    """how a launch relates its strides to its sizes: which axis of A and of B is contiguous and whether the other stride equals that
    axis' length (a compact operand) or exceeds it (a view); the same for C; accumulate; bias.  "<" never occurs in a sound launch."""
    a = "k" + _rel(sam, K) if sak == 1 else "m" + _rel(sak, M) if sam == 1 else "?"
    b = "n" + _rel(sbk, N) if sbn == 1 else "k" + _rel(sbn, K) if sbk == 1 else "?"
    return a, b, "c" + _rel(ldc, N), bool(acc), bool(bias)


def _case_signature(c):
    return _signature(c["sam"], c["sak"], c["sbk"], c["sbn"], c["ldc"], c["M"], c["N"], c["K"], c["acc"], c["bias"] is not None)


@pytest.mark.parametrize("case", GEMM_CASES, ids=[c["name"] for c in GEMM_CASES])
def test_gemm_as_launched(case):
    c = case
    M, N, K = c["M"], c["N"], c["K"]
    rng = np.random.RandomState(M + 7 * N + 13 * K + len(c["name"]))
    fa, _da, A, ma = _place(rng, *c["A"])
    fb, _db, B, mb = _place(rng, *c["B"])
    fc, _dc, C, mc = _place(rng, *c["C"])
    _ia, a = _addressed(fa, ma, A.storage_offset(), M, c["sam"], K, c["sak"], "A")
    _ib, b = _addressed(fb, mb, B.storage_offset(), K, c["sbk"], N, c["sbn"], "B")
    ic, c0 = _addressed(fc, mc, C.storage_offset(), M, c["ldc"], N, 1, "C")
    bias, bias_t = np.zeros(N, dtype=np.float32), None
    if c["bias"] is not None:
        fbias, _dbias, bias_t, mbias = _place(rng, c["bias"][0], c["bias"][1])
        bias = fbias[mbias]
        assert bias.shape == (N,) and bias_t.storage_offset() == LEAD + (c["bias"][1].start or 0)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    exact = a64 @ b64 + bias + (c0 if c["acc"] else 0.0)
    bound = 1.01 * (K + 2) * U * (np.abs(a64) @ np.abs(b64) + np.abs(bias) + np.abs(c0))
    O = jops.backend()
    outs = []
    for _ in range(2):
        _dc.copy_(torch.from_numpy(fc))
        O.train_gemm(A, c["sam"], c["sak"], B, c["sbk"], c["sbn"], C, c["ldc"], M, N, K, c["acc"], bias_t)
        outs.append(_dc.cpu().numpy())
    got = outs[0]
    err = np.abs(got[ic] - exact)
    assert np.isfinite(got[ic]).all(), "a read outside the operands' views"
    print("%s: signature %s, worst |error| / bound %.3f" % (c["name"], _case_signature(c), float((err / bound).max())))
    assert np.all(err <= bound), (c["name"], float((err / bound).max()))
    assert np.array_equal(_bits(got[~mc]), _bits(fc[~mc])), "C's storage outside the [M, N] window was written"
    assert np.array_equal(_bits(outs[1]), _bits(got))                      # the same bits, launch after launch


class _Recorder:
    """jlm_amd.ops' backend with every train_gemm launch noted on its way through"""

    def __init__(self, ops):
        self._ops, self.calls = ops, []

    def __getattr__(self, name):
        return getattr(self._ops, name)

    def train_gemm(self, A, sam, sak, B, sbk, sbn, C, ldc, M, N, K, acc, bias):
        self.calls.append(dict(sam=sam, sak=sak, sbk=sbk, sbn=sbn, ldc=ldc, M=M, N=N, K=K, acc=bool(acc), bias=bias,
                               a_off=A.storage_offset(), a_words=A.untyped_storage().nbytes() // 4, c_off=C.storage_offset()))
        return self._ops.train_gemm(A, sam, sak, B, sbk, sbn, C, ldc, M, N, K, acc, bias)


@pytest.mark.parametrize("mode", ["tied", "vtable", "dsoftmax"])
@pytest.mark.parametrize("chunk_bytes", [ONE_WINDOW, WINDOWS_OF_64], ids=["one-window", "windows-of-64"])
def test_gemm_cases_cover_the_step(mode, chunk_bytes):
    """every train_gemm launch of a step of the odd model at N = 35 relates its strides to its sizes as one of GEMM_CASES does, and the
    forms the cases were written for are launched: a new or changed launch in step_async needs its case"""
    cfg = tc.odd_cfg(mode, True)
    dev = T.DeviceStepper(cfg, T.init_weights(cfg, None, 101), NB, NT, dropout=0.9, seed=42, chunk_bytes=chunk_bytes)
    dev.ops = rec = _Recorder(dev.ops)
    dev.step(*tc.batch(V, NB, NT, 3))
    table = {_case_signature(c) for c in GEMM_CASES}
    seen = {}
    for call in rec.calls:
        sig = _signature(call["sam"], call["sak"], call["sbk"], call["sbn"], call["ldc"], call["M"], call["N"], call["K"], call["acc"],
                         call["bias"] is not None)
        seen.setdefault(sig, call)
    print("%s, Vc = %d: %d train_gemm launches, %d stride / size relations" % (mode, dev.Vc, len(rec.calls), len(seen)))
    missing = {sig: {k: v for k, v in call.items() if k != "bias"} for sig, call in seen.items() if sig not in table}
    assert not missing, missing
    Em = dev.d["E"]

    def launched(**want):
        return any(all(call[k] == v for k, v in want.items()) for call in rec.calls)
    # the recurrent products on row-offset views, HM read transposed; dHM over the first N rows of the (T + 1) B-row buffer
    assert any(c["a_off"] > 0 and c["c_off"] > 0 and c["acc"] for c in rec.calls if (c["M"], c["N"], c["K"]) == (NB, H4, H))
    assert any(c["a_off"] > 0 for c in rec.calls if (c["sbk"], c["sbn"], c["M"], c["N"], c["K"]) == (1, H4, NB, H, H4))
    assert any(c["a_words"] == (NT + 1) * NB * H for c in rec.calls if (c["sam"], c["sak"], c["M"], c["N"], c["K"]) == (1, H, H, H4, NR))
    if chunk_bytes == WINDOWS_OF_64:
        assert dev.Vc == 64
        if mode != "tied":                                                          # a piece inside a window: C and b2 start at an odd word
            assert any(c["bias"] is not None and c["bias"].storage_offset() % 2 == 1 and c["c_off"] % 64 for c in rec.calls if c["ldc"] == 64)
        assert launched(sam=1, sak=64, K=NR)                                        # dBlock = dy^T Q
    if mode == "dsoftmax":
        assert launched(sam=Em, sak=1, K=5, sbk=1, sbn=5) and launched(ldc=Em, N=5, acc=False)
        assert launched(ldc=Em, N=5, acc=True) == (chunk_bytes == WINDOWS_OF_64)    # dQ += dy Block on columns of dP
    if mode == "vtable":
        assert launched(sam=1, sak=9, M=9, N=Em, K=NR, acc=False)                   # dVT_i = dQ_i^T P
        assert launched(sam=1, sak=9, M=9, N=Em, K=53, acc=True)                    # dVT_i += LM_i^T D


# ---- 2. one step at odd sizes, on all three embeddings
STEP_KW = dict(lr=1e-3, norm_weight=0.1, seed=42)
PADDED = {"tied": {"b2", "PM", "LM"}, "vtable": {"b2", "PM", "LM1", "VT1", "VT2"}, "dsoftmax": {"b2", "PM", "LM"}}
_weights, _references = {}, {}


def _odd_model(mode, self_norm):
    if (mode, self_norm) not in _weights:
        cfg = tc.odd_cfg(mode, self_norm)
        _weights[(mode, self_norm)] = (cfg, T.init_weights(cfg, None, 101))
    return _weights[(mode, self_norm)]


def _reference_step(key, cfg, w, B, Tn, keep, x, y, h0, c0):
    """the restatement's step, computed once per case and shared by the budgets it is run at"""
    if key not in _references:
        ref = T.ReferenceStepper(cfg, w, B, Tn, dropout=keep, **STEP_KW)
        ref.set_state(h0, c0)
        ce = ref.step(x, y)
        _references[key] = dict(ce=ce, grads=ref.grads(), h=ref.h.copy(), c=ref.c.copy(), w=T._map(ref.w, np.copy))
    return _references[key]


def _check_padding(dev, pad, names):
    for name in names:
        assert not getattr(dev, name).cpu().numpy()[pad].any(), "the padding of %s is not zero" % name


def _poison_scratch(dev):
    """NaN in every buffer a step has to write before it reads it (all but the parameters, the carried state, the loss slots, and the
    dense Emb, whose zeros a D_softmax model reads): a launch that reads what this step did not write -- ``dh`` at the last time
    step, where no ``dh`` product has run -- shows in the gradients"""
    bufs = [dev.X, dev.dX, dev.P, dev.dP, dev.Z, dev.dZ, dev.R, dev.dR, dev.dc, dev.dh, dev.run_m, dev.run_s, dev.tgt, dev.Y,
            dev.Hs[dev.B:], dev.Cs[dev.B:]]
    for b in bufs + list(dev.Q.values()) + list(dev.dQ.values()) + list(dev.D.values()):
        b.fill_(NAN)


def _step_case(key, cfg, w, B, Tn, keep, chunk_bytes=ONE_WINDOW, same_word=None):
    Vn, Hn = int(np.asarray(w["b2"]).shape[0]), cfg["hidden_size"]
    x, y = tc.batch(Vn, B, Tn, 3)
    if same_word is not None:
        x[:] = same_word
    h0, c0 = tc.carried_state(B, Hn, 4)
    want = _reference_step(key, cfg, w, B, Tn, keep, x, y, h0, c0)
    dev = T.DeviceStepper(cfg, w, B, Tn, dropout=keep, chunk_bytes=chunk_bytes, **STEP_KW)
    pad = tc.padding_mask(dev.layout, dev.n_flat)
    dev.set_state(h0, c0)
    _poison_scratch(dev)
    ce = dev.step(x, y)
    worst = tc.worst_relative(dev.grads(), want["grads"])
    dh = np.abs(dev.Hs[:B].cpu().numpy() - want["h"]).max() / U
    dc = np.abs(dev.Cs[:B].cpu().numpy() - want["c"]).max() / U
    dw = max(float(np.abs(a.astype(np.float64) - b).max()) for (_k, a), (_k2, b) in zip(tc.flat_items(dev.weights()), tc.flat_items(want["w"])))
    print("%s Vc %d: |ce_dev - ce_ref| %.2e; h, c off by %.1f u, %.1f u; weights by %.2e lr; worst relative gradient deviation %.2e (%s) of %s"
          % (key, dev.Vc, abs(ce - want["ce"]), dh, dc, dw / STEP_KW["lr"], max(worst.values()), max(worst, key=worst.get),
             {k: "%.1e" % v for k, v in worst.items()}))
    assert abs(ce - want["ce"]) <= 1e-5, (ce, want["ce"])
    for k, v in worst.items():
        assert v <= 1e-4, (k, v)
    assert dh <= 32 and dc <= 32
    assert dw <= STEP_KW["lr"] * 1e-3
    _check_padding(dev, pad, ("G", "W", "M", "Vv"))
    assert dev.t == 1
    return dev, pad


@pytest.mark.parametrize("mode", ["tied", "vtable", "dsoftmax"])
@pytest.mark.parametrize("self_norm", [False, True], ids=["plain", "self-norm"])
@pytest.mark.parametrize("B,Tn,keep", [(7, 5, 0.9), (1, 1, 0.9), (3, 1, 1.0), (1, 4, 0.9), (5, 3, 1.0)])
def test_step_at_odd_sizes(mode, self_norm, B, Tn, keep):
    cfg, w = _odd_model(mode, self_norm)
    dev, pad = _step_case((mode, self_norm, B, Tn, keep), cfg, w, B, Tn, keep)
    assert dev.Vc == V and len(dev._windows()) == 1
    padded = {key for key, _idx, _shape, _off, n in dev.layout if n % 4}
    assert padded == PADDED[mode] and pad.sum() == sum(-n % 4 for _k, _i, _s, _o, n in dev.layout)


@pytest.mark.parametrize("mode", ["tied", "vtable", "dsoftmax"])
@pytest.mark.parametrize("self_norm", [False, True], ids=["plain", "self-norm"])
def test_step_at_odd_sizes_in_windows_of_64(mode, self_norm):
    """Vc at its floor: windows of 64, 64 and 29 words, which cut segments 1 and 2 and put two segments into one window"""
    cfg, w = _odd_model(mode, self_norm)
    dev, _pad = _step_case((mode, self_norm, 7, 5, 0.9), cfg, w, 7, 5, 0.9, chunk_bytes=WINDOWS_OF_64)
    assert dev.Vc == 64
    assert [n for _v0, n, _pieces in dev._windows()] == [64, 64, 29]
    if mode != "tied":
        assert [[si for si, _a, _n in pieces] for _v0, _n, pieces in dev._windows()] == [[0, 1], [1, 2], [2]]


@pytest.mark.parametrize("mode", ["tied", "vtable", "dsoftmax"])
def test_step_with_one_input_word(mode):
    """every input id is word 17: the scatter sees one run of N rows, the other N-row products identical rows"""
    cfg, w = _odd_model(mode, True)
    _step_case((mode, "one word"), cfg, w, 7, 5, 0.9, same_word=17)


def test_step_of_the_character_model():
    """the softmax runs over n_out = 37 characters, not vocab_size words (tests/test_train_cpu.py's character case)"""
    cfg = tc.small_cfg("tied", 600, 24, 12, True, char_rnn=True)
    w = T.init_weights(cfg, 37, 3)
    dev, pad = _step_case(("char",), cfg, w, 6, 4, 0.9)
    assert dev.d["V"] == 37 and pad.sum() == 3                  # b2's 37 words are padded to 40


# ---- 3. the evaluation pass and the state it carries
def _last_ce(dev):
    return dev.ce[dev.n_ce - 1:dev.n_ce].cpu().numpy()


@pytest.mark.parametrize("mode", ["vtable", "tied"])
def test_eval_pass_and_carried_state(mode):
    """train, eval, eval, train, eval without a reset: an eval step uses keep = 1 whatever ``dropout`` is, leaves the weights, the Adam
    moments and the step counter alone, and hands its state on.  ``win`` runs every eval step once more from the same weights and
    state in windows of 64 words: there train_dy meets a half-built normaliser, which must not reach the target's logit."""
    cfg, w = _odd_model(mode, True)
    B, Tn = 7, 5
    kw = dict(lr=1e-3, dropout=0.9, norm_weight=0.1, seed=42)
    ref, dev = T.ReferenceStepper(cfg, w, B, Tn, **kw), T.DeviceStepper(cfg, w, B, Tn, **kw)
    win = T.DeviceStepper(cfg, w, B, Tn, chunk_bytes=WINDOWS_OF_64, **kw)
    assert (dev.Vc, win.Vc) == (V, 64)
    h0, c0 = tc.carried_state(B, H, 4)
    ref.set_state(h0, c0)
    dev.set_state(h0, c0)
    for i, train in enumerate([True, False, False, True, False]):
        x, y = tc.batch(V, B, Tn, 20 + i)
        if not train:
            for mine, theirs in ((win.W, dev.W), (win.Hs[:B], dev.Hs[:B]), (win.Cs[:B], dev.Cs[:B])):
                mine.copy_(theirs)
            before = [a.clone() for a in (dev.W, dev.M, dev.Vv)]
        ref.step_async(x, y, train)
        dev.step_async(x, y, train)
        if train:
            worst = tc.worst_relative(dev.grads(), ref.grads())
            print("step %d (train): worst relative gradient deviation %.2e" % (i, max(worst.values())))
            assert max(worst.values()) <= 1e-4, worst
        else:
            win.step_async(x, y, False)
            assert all(torch.equal(a, b) for a, b in zip(before, (dev.W, dev.M, dev.Vv))), "an eval step changed the weights or the moments"
            assert torch.equal(win.tgt, dev.tgt), "the target's logit depends on the windows"
            print("step %d (eval): ce %.9f in one window, %.9f in windows of 64" % (i, _last_ce(dev)[0], _last_ce(win)[0]))
            assert abs(_last_ce(win)[0] - ref.losses()[-1]) <= 1e-5
        for got, want in ((dev.Hs[:B], ref.h), (dev.Cs[:B], ref.c)):
            assert np.abs(got.cpu().numpy() - want).max() <= 32 * U
    a, b = ref.losses(), dev.losses()
    print("%s: |ce_dev - ce_ref| over train, eval, eval, train, eval: %s" % (mode, ["%.1e" % v for v in np.abs(a - b)]))
    assert len(b) == 5 and np.abs(a - b).max() <= 1e-5
    assert dev.t == ref.t == 2
    ref.reset_state()
    dev.reset_state()
    x, y = tc.batch(V, B, Tn, 30)
    ce_ref, ce_dev = ref.step(x, y, train=False), dev.step(x, y, train=False)
    assert abs(ce_ref - ce_dev) <= 1e-5 and len(dev.losses()) == 1 and dev.t == 2


@pytest.mark.parametrize("mode", ["vtable", "tied"])
def test_eval_ce_has_the_same_bits_in_windows_of_64(mode):
    """Two eval steps from the same weights and state, once with the whole vocabulary in one window and once in windows of 64 words:
    the targets' logits, the rows' normalisers and the ce are the same bits.  ``lse_update_kernel`` meets a window in granules of 64
    words and merges them in order, and Vc is a multiple of 64, so the cut into windows does not enter the normaliser.  (Before that
    a window's sum was one lane-strided pass and the windows' pairs were merged afterwards: 1 to 2 of these 35 rows' normalisers
    differed by up to 2 ulp between the two budgets, the ce by 2e-8.)"""
    cfg, w = _odd_model(mode, True)
    B, Tn = 7, 5
    kw = dict(lr=1e-3, dropout=0.9, norm_weight=0.1, seed=42)
    one, win = T.DeviceStepper(cfg, w, B, Tn, **kw), T.DeviceStepper(cfg, w, B, Tn, chunk_bytes=WINDOWS_OF_64, **kw)
    h0, c0 = tc.carried_state(B, H, 4)
    for st in (one, win):
        st.set_state(h0, c0)
        for i in range(2):
            st.step_async(*tc.batch(V, B, Tn, 20 + i), train=False)
    assert torch.equal(one.tgt, win.tgt)
    lse = [(st.run_m + torch.log(st.run_s)).cpu().numpy() for st in (one, win)]
    a, b = one.losses(), win.losses()
    print("%s: eval ce in one window %s, in windows of 64 %s; %d of %d rows' normalisers differ, by at most %.1f ulp"
          % (mode, a, b, int((lse[0] != lse[1]).sum()), B * Tn, float(np.abs(lse[0] - lse[1]).max() / np.spacing(np.abs(lse[0]).max()))))
    assert np.array_equal(_bits(lse[0]), _bits(lse[1]))
    assert _bits(a.astype(np.float64)).tolist() == _bits(b.astype(np.float64)).tolist()


# ---- 4. more than 256 steps between two read-backs
def test_three_hundred_steps_without_a_read_back():
    """the loss buffer holds 256 steps and is doubled while earlier steps are in flight: the first 256 entries must survive"""
    cfg = tc.small_cfg("tied", 600, 24, 12, True, char_rnn=True)
    w = T.init_weights(cfg, 37, 3)
    kw = dict(lr=1e-3, dropout=0.9, norm_weight=0.1, seed=5)
    ref, dev = T.ReferenceStepper(cfg, w, 2, 1, **kw), T.DeviceStepper(cfg, w, 2, 1, **kw)
    rng = np.random.RandomState(6)
    xs, ys = rng.randint(0, 37, (300, 2, 1)), rng.randint(0, 37, (300, 2, 1))
    for x, y in zip(xs, ys):
        ref.step_async(x, y, False)
        dev.step_async(x, y, False)
    assert dev.ce.numel() == 512
    a, b = ref.losses(), dev.losses()
    assert len(b) == 300
    print("300 eval steps, B = 2, T = 1: largest |ce_dev - ce_ref| %.2e (first 256: %.2e)" % (np.abs(a - b).max(), np.abs(a - b)[:256].max()))
    assert np.abs(a - b).max() <= 1e-5
    assert len(np.unique(b)) > 250                               # the entries are the steps' own, not one value repeated
    ref.reset_state()
    dev.reset_state()
    assert abs(ref.step(xs[0], ys[0], train=False) - dev.step(xs[0], ys[0], train=False)) <= 1e-5
    assert len(dev.losses()) == 1 and dev.t == 0


# ---- 5. fine-tuning at the same sizes
_ft_models = {}


def _ft_model(mode, bit):
    if (mode, bit) not in _ft_models:
        cfg, w = _odd_model(mode, True)
        pairs = {k: tc.grid_quantise(v, 1 << bit) for k, v in w.items()}
        _ft_models[(mode, bit)] = (cfg, {k: c for k, (c, _b) in pairs.items()}, {k: b for k, (_c, b) in pairs.items()})
    return _ft_models[(mode, bit)]


@pytest.mark.parametrize("mode", ["vtable", "tied"])
@pytest.mark.parametrize("bit", [1, 3])
@pytest.mark.parametrize("B,Tn", [(7, 5), (1, 1)])
def test_finetune_step_at_odd_sizes(mode, bit, B, Tn):
    """tests/test_gpu_finetune.py::test_one_step on the odd model: the layout pads tensors, so gid = -1 comes from build_groups, and at
    bit = 1 the V_table model's 19 tensors x 2 codes = 38 groups pad the codebook buffer to 40"""
    cfg, codes, books = _ft_model(mode, bit)
    kw = dict(lr=1e-3, dropout=0.9, norm_weight=0.1, seed=42)
    ref = F.CodebookReferenceStepper(cfg, codes, books, B, Tn, **kw)
    dev = F.CodebookDeviceStepper(cfg, codes, books, B, Tn, **kw)
    pad = tc.padding_mask(dev.layout, dev.n_flat)
    assert pad.any() and np.array_equal(dev.gid.cpu().numpy() == -1, pad)
    assert dev.n_groups == len(codes) << bit and dev.n_book == (dev.n_groups + 3) // 4 * 4
    if (mode, bit) == ("vtable", 1):
        assert (dev.n_groups, dev.n_book) == (38, 40)
    tc.codebook_image(dev)
    for k in codes:
        assert dev.codebooks()[k].tobytes() == books[k].tobytes()
    h0, c0 = tc.carried_state(B, H, 4)
    ref.set_state(h0, c0)
    dev.set_state(h0, c0)
    x, y = tc.batch(V, B, Tn, 3)
    ce_ref, ce_dev = ref.step(x, y), dev.step(x, y)
    want, got = ref.codebook_grads(), dev.codebook_grads()
    worst = {k: float(np.abs(got[k] - want[k]).max() / np.abs(want[k]).max()) for k in want}
    print("%s, %d bit, B = %d, T = %d: |ce_dev - ce_ref| %.2e, worst relative codebook-gradient deviation %.1e (%s)"
          % (mode, bit, B, Tn, abs(ce_ref - ce_dev), max(worst.values()), max(worst, key=worst.get)))
    assert abs(ce_ref - ce_dev) <= 1e-5, (ce_ref, ce_dev)
    for k, v in worst.items():
        assert v <= 1e-4, (k, v)
    tc.codebook_image(dev)
    assert any(dev.codebooks()[k].tobytes() != books[k].tobytes() for k in codes)
    for k in codes:
        assert np.array_equal(dev.codes()[k], codes[k])
    _check_padding(dev, pad, ("G", "W"))
    for name in ("book", "gbook", "bm", "bv"):
        assert not getattr(dev, name)[dev.n_groups:].cpu().numpy().any(), "the padding tail of %s is not zero" % name
