"""GPU: the kernels dynamic evaluation adds to csrc/jlm_train.hip, each on its own: ``train_gemm_splitk`` (the contraction cut into
pieces of kc, the pieces' tiles added in order), ``dyneval_sqacc``, ``dyneval_rms`` and ``dyneval_update``.

The split product is held to the bar of tests/test_gpu_train_shapes.py::test_gemm_as_launched, 1.01 (K + 2) u (|A| |B| + |bias| + |C|)
with u = 2^-24: a piece's fmaf chain has at most kc terms and the S pieces take S - 1 additions, and kc + S - 1 <= K wherever there is
more than one piece.  Beyond the bar its bits are pinned: they are those of ``train_gemm`` over each piece of the contraction, added in
float32 in piece order, then the bias, then C.  The flat-buffer kernels are held to 2 ulp of the float64 formula per element."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
from jlm_amd import _lib, ops as jops                                       # noqa: E402

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
NAN = float("nan")
KC = 16
FORMS = {            # how A [M, K] and B [K, N] lie in memory: (A is stored transposed, B is stored transposed)
    "NT": (False, True), "TN": (True, False), "NN": (False, False)}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _operands(rng, form, M, N, K):
    """-> (a [M, K], b [K, N] as numbers, the device storages and their strides (sam, sak, sbk, sbn))"""
    ta, tb = FORMS[form]
    a, b = rng.normal(size=(M, K)).astype(np.float32), rng.normal(size=(K, N)).astype(np.float32)
    A, sa = (_dev(a.T), (1, M)) if ta else (_dev(a), (K, 1))
    Bm, sb = (_dev(b.T), (1, K)) if tb else (_dev(b), (N, 1))
    return a, b, A, sa, Bm, sb


@pytest.mark.parametrize("K", [1, 16, 17, 49])
@pytest.mark.parametrize("M,N", [(5, 19), (64, 64), (65, 65)])
def test_split_gemm(M, N, K):
    O = jops.backend()
    S = -(-K // KC)
    ldc = N + 3
    worst = 0.0
    for fi, form in enumerate(FORMS):
        for acc in (False, True):
            for with_bias in (False, True):
                rng = np.random.RandomState(1000 * fi + 100 * acc + 10 * with_bias + M + N + K)
                a, b, A, sa, Bm, sb = _operands(rng, form, M, N, K)
                c0 = rng.normal(size=(M, ldc)).astype(np.float32)
                bias = rng.normal(size=N).astype(np.float32) if with_bias else None
                bias_t = _dev(bias) if with_bias else None
                outs = []
                for _run in range(2):
                    C = _dev(c0)
                    part = torch.full((S * M * N + 8,), NAN, device="cuda")
                    O.train_gemm_splitk(A, sa[0], sa[1], Bm, sb[0], sb[1], C, ldc, M, N, K, acc, bias_t, KC, part)
                    outs.append(C.cpu().numpy())
                    assert torch.isnan(part[S * M * N:]).all(), "part was written past S M N"
                    assert not torch.isnan(part[:S * M * N]).any()
                got = outs[0]
                assert np.array_equal(_bits(outs[1]), _bits(got)), "two runs differ"
                assert np.array_equal(_bits(got[:, N:]), _bits(c0[:, N:])), "C was written outside its [M, N] window"
                a64, b64 = a.astype(np.float64), b.astype(np.float64)
                bz = bias if with_bias else np.zeros(N, dtype=np.float32)
                exact = a64 @ b64 + bz + (c0[:, :N] if acc else 0.0)
                bound = 1.01 * (K + 2) * U * (np.abs(a64) @ np.abs(b64) + np.abs(bz) + np.abs(c0[:, :N]))
                err = np.abs(got[:, :N] - exact)
                worst = max(worst, float((err / bound).max()))
                assert np.all(err <= bound), (form, acc, with_bias, float((err / bound).max()))
                # the bits: train_gemm over each piece, added in piece order in float32, then the bias, then C
                want = None
                for s in range(S):
                    lo, hi = s * KC, min(K, (s + 1) * KC)
                    piece = torch.full((M, N), NAN, device="cuda")
                    Ao = A[lo:hi] if FORMS[form][0] else A[:, lo:hi]
                    Bo = Bm[:, lo:hi] if FORMS[form][1] else Bm[lo:hi]
                    O.train_gemm(Ao, sa[0], sa[1], Bo, sb[0], sb[1], piece, N, M, N, hi - lo, False, None)
                    p = piece.cpu().numpy()
                    want = p if want is None else (want + p).astype(np.float32)
                if with_bias:
                    want = (want + bias).astype(np.float32)
                if acc:
                    want = (want + c0[:, :N]).astype(np.float32)
                assert np.array_equal(_bits(got[:, :N]), _bits(want)), (form, acc, with_bias)
                if S == 1:                                   # K <= kc: the one launch of train_gemm itself
                    C = _dev(c0)
                    O.train_gemm(A, sa[0], sa[1], Bm, sb[0], sb[1], C, ldc, M, N, K, acc, bias_t)
                    assert np.array_equal(_bits(C.cpu().numpy()), _bits(got))
    print("M %d N %d K %d (%d pieces of %d): worst |error| / bound %.3f" % (M, N, K, S, KC, worst))


def test_split_gemm_refuses_a_short_part():
    O, L = jops.backend(), _lib.lib()
    M, N, K = 5, 19, 49
    S = -(-K // KC)
    rng = np.random.RandomState(0)
    _a, _b, A, sa, Bm, sb = _operands(rng, "NN", M, N, K)
    C = torch.full((M, N), 7.0, device="cuda")
    part = torch.full((S * M * N,), NAN, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    args = (A.data_ptr(), sa[0], sa[1], Bm.data_ptr(), sb[0], sb[1], C.data_ptr(), N, M, N, K, 0, None, KC, part.data_ptr())
    assert L.jlm_train_gemm_splitk(*args, S * M * N - 1, st) == -1
    assert L.jlm_train_gemm_splitk(*args[:13], 24, part.data_ptr(), S * M * N, st) == -1          # kc is no multiple of 16
    torch.cuda.synchronize()
    assert bool((C == 7.0).all()) and bool(torch.isnan(part).all()), "a refused call launched something"
    with pytest.raises(RuntimeError):
        O.train_gemm_splitk(A, sa[0], sa[1], Bm, sb[0], sb[1], C, N, M, N, K, False, None, KC, part[:-1])
    assert L.jlm_train_gemm_splitk(*args, S * M * N, st) == 0
    torch.cuda.synchronize()
    assert not bool(torch.isnan(C).any()) and not bool((C == 7.0).all())


# ---- the flat-buffer kernels.  n = 4: one 16-byte access; n = 4 (256 4096) + 4: the grid is capped at 4096 blocks of 256 lanes, so the
# last access is the first lane's second trip through the grid-stride loop
SIZES = [4, 4 * (256 * 4096) + 4]


def _ulp32(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def _flat(rng, n, scale, pad=3):
    """n float32 with the last ``pad`` words zero, as the flat parameter buffer's padding is"""
    a = rng.normal(0, scale, n).astype(np.float32)
    a[n - pad:] = 0.0
    return a


@pytest.mark.parametrize("n", SIZES)
def test_sqacc_and_rms(n):
    O = jops.backend()
    rng = np.random.RandomState(n % 97)
    g, ms0 = _flat(rng, n, 1e-2), np.abs(_flat(rng, n, 1e-4))
    g[5::5] = 0.0
    ms0[5::5] = 0.0                                               # elements whose RMS is exactly 0
    ms, flag = _dev(ms0), torch.zeros(1, dtype=torch.int32, device="cuda")
    O.dyneval_sqacc(ms, _dev(g), n, flag)
    got = ms.cpu().numpy()
    exact = g.astype(np.float64) ** 2 + ms0
    assert np.all(np.abs(got - exact) <= 2 * _ulp32(exact))
    assert not got[n - 3:].any() and not got[5::5].any()                          # padding stays 0
    flag.fill_(1)
    O.dyneval_sqacc(ms, _dev(g), n, flag)
    assert np.array_equal(_bits(ms.cpu().numpy()), _bits(got)), "a raised flag did not stop the accumulation"
    # rms and its mean over the n - 3 real values
    inv = 1.0 / 7
    rms = torch.full((n,), NAN, device="cuda")
    partial = torch.full((4096,), NAN, dtype=torch.float64, device="cuda")
    mean = torch.full((1,), NAN, dtype=torch.float64, device="cuda")
    O.dyneval_rms(ms, n, inv, rms, n - 3, partial, mean)
    r = rms.cpu().numpy()
    exact = np.sqrt(got.astype(np.float64) * float(np.float32(inv)))
    assert np.all(np.abs(r - exact) <= 2 * _ulp32(exact)) and not r[n - 3:].any() and not r[5::5].any()
    want = r[:n - 3].astype(np.float64).mean()
    assert abs(float(mean.item()) - want) <= 1e-12 * want, (float(mean.item()), want)
    again = torch.full((1,), NAN, dtype=torch.float64, device="cuda")
    O.dyneval_rms(ms, n, inv, torch.empty_like(rms), n - 3, torch.full_like(partial, NAN), again)
    assert again.cpu().numpy().tobytes() == mean.cpu().numpy().tobytes()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("rule,lr,lam", [("sgd", 0.05, 0.0), ("sgd", 0.005, 0.02), ("rms", 1e-3, 0.02), ("rms", 1e-3, 0.0), ("rms", 3e-4, 0.9)])
def test_update(n, rule, lr, lam):
    """the float64 formula of jlm_amd.dyneval.DynEvalReferenceStepper on the same float32 operands; the kernel evaluates it in f64 and
    rounds once, so 2 ulp of the result leaves room"""
    O = jops.backend()
    rng = np.random.RandomState(n % 89 + len(rule))
    w0 = _flat(rng, n, 0.1)
    w = (w0 + _flat(rng, n, 1e-2)).astype(np.float32)
    g = _flat(rng, n, 1e-2)
    eps = 1e-3
    rms = None
    if rule == "rms":
        rms = np.abs(_flat(rng, n, 1e-2))
        rms[5::5] = 0.0                                           # RMS = 0: the step is lr g / eps, the decay coefficient 0
        rms[1::11] = 5.0                                          # and a coefficient that the min() caps at 1
        rms[n - 3:] = 0.0
        scale = lam / rms[:n - 3].astype(np.float64).mean()
        w64, g64, r64 = w.astype(np.float64), g.astype(np.float64), rms.astype(np.float64)
        exact = w64 - lr * g64 / (r64 + eps) + np.minimum(scale * r64, 1.0) * (w0 - w64)
        assert n == 4 or lam < 0.9 or (np.minimum(scale * r64, 1.0) == 1.0).any()
    else:
        scale = lam
        w64 = w.astype(np.float64)
        exact = w64 - lr * g.astype(np.float64) + lam * (w0 - w64)
    W, flag = _dev(w), torch.zeros(1, dtype=torch.int32, device="cuda")
    flag.fill_(1)
    O.dyneval_update(W, _dev(g), _dev(w0), None if rms is None else _dev(rms), n, lr, scale, eps, flag)
    assert np.array_equal(_bits(W.cpu().numpy()), _bits(w)), "a raised flag did not stop the update"
    flag.zero_()
    O.dyneval_update(W, _dev(g), _dev(w0), None if rms is None else _dev(rms), n, lr, scale, eps, flag)
    got = W.cpu().numpy()
    err = np.abs(got - exact) / _ulp32(exact)
    print("%s lr %g lam %g, n %d: worst error %.2f ulp" % (rule, lr, lam, n, float(err.max())))
    assert np.all(err <= 2)
    assert not got[n - 3:].any(), "the padding moved"
    assert not np.array_equal(got[:n - 3], w[:n - 3])
