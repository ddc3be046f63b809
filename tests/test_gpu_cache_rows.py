"""GPU: cache_rows_kernel as jlm_cache_rows launches it (csrc/jlm_cache.hip, include/jlm_hip.h), on rings the test writes -- no model.
Every lpc is checked against the definition in float64 over the DECODED operands (split rows: (hi + lo) / h_scale), within a bar that
is derived here, not measured.

The bar.  u = 2^-24.  For a query q and an entry i, A_i = sum_k |q_k| |k_k| (real units).

  products      split rows: three v_mfma_f32_32x32x16_f16 per 16 k into one f32 accumulator.  Every product of two f16 halves is exact
                in f32; an instruction adds its 16 products with at most 2 ulp(C) <= 2^-22 |C| of error and |C| never
                exceeds the sum of the |terms| <= (1 + 2^-10) A_i (the cross terms hi.lo, lo.hi add at most 2 * 2^-11 A_i); 3 H / 16
                instructions; the dropped lo.lo is at most 2^-22 A_i:        E_split(H) = (3 H / 16) 2^-22 (1 + 2^-9) + 2^-22
                f32 rows: v_mfma_f32_32x32x2_f32 is a k-ordered fmaf chain of H terms:  E_f32(H) = H u / (1 - H u)
  scores        s_i = f32(theta' * dot) (theta' = theta / h_scale^2, exact: a power of two) and the f32 difference s_i - m with
                |s_i - m| <= 2 theta max_i A_i add 3 u theta A:
                    |delta s_i| <= DS = theta * max_i A_i * (E(H) + 4 u)
  lpc           log sum exp is 1-Lipschitz in the largest |delta s_i|, once for log M and once for log Z:     2 DS
  the sums      M and Z are f32 sums of at most N positive terms: expf is within 1 ulp (2 u relative) per term, at most N - 1
                effective additions (u each, of positive partial sums; adding an empty partial sum is exact), and a partial sum is
                rescaled by expf(m_old - m_new) once per stage it passes (3 u: the expf and the product) -- at most
                2 ceil(ceil((N + 62) / 32) / 16) tile stages of a wave, the half-wave fold and the eight-wave fold:
                    ES = (2 + N + 3 (stages + 2)) u * 1.01          on log M and on log Z each
  logf          within 1 ulp of its result, and the final f32 subtraction:   2 u (|log M| + |log Z|) + u |lpc|  (reference values,
                log Z and log M taken under the running maximum as the kernel takes them, + 2 u for results near 0)

  BAR_q = 2 DS + 2 ES + 2 u (|log M| + |log Z| + 1) + u |lpc|

It holds while the largest matching term stays inside the f32 exponent range under the running maximum (s_match - m > -80: asserted
of every case's reference, so no case is tested where f32 itself gives out).  Exact values are asserted where the definition gives
them: -inf without a match, 0.0 when every entry matches (M and Z are then the same sums, bit for bit), entries the row does not have
left untouched, theta independent of its neighbours bit for bit.  The formulas live in tests/cache_budget.py (kernel_bar), shared with tests/test_gpu_cache.py.  Measured maxima: DESIGN.md section 18.
"""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
from jlm_amd import _lib                                                                  # noqa: E402
from tests.cache_budget import U, kernel_bar                                              # noqa: E402

pytestmark = pytest.mark.gpu

H_SCALE = 2.0 ** 14
FILL = 123.0                                                                               # what lpc holds before a launch
NAN_BITS = np.float32(np.nan)


def encode(x, split):
    """real-valued rows [..., H] f32 -> (raw float32 bits in the state-row format, the decoded float64 values)"""
    x = np.asarray(x, dtype=np.float32)
    if not split:
        return x.copy(), x.astype(np.float64)
    s = x * np.float32(H_SCALE)
    hi = s.astype(np.float16)
    lo = (s - hi.astype(np.float32)).astype(np.float16)
    H = x.shape[-1]
    blk = lambda a: a.reshape(x.shape[:-1] + (H // 8, 1, 8))
    raw = np.concatenate([blk(hi), blk(lo)], axis=-2).reshape(x.shape[:-1] + (2 * H,)).view(np.float32)
    return np.ascontiguousarray(raw), (hi.astype(np.float64) + lo.astype(np.float64)) / H_SCALE


class Rings:
    """host rings [cap][R][H] / [cap][R], NaN / -1 where nothing exists; put() writes position p of row r"""

    def __init__(self, cap, R, H, split):
        self.cap, self.R, self.H, self.split = cap, R, H, split
        self.raw = np.full((cap, R, H), NAN_BITS, dtype=np.float32)
        self.val = np.full((cap, R, H), np.nan)
        self.words = np.full((cap, R), -1, dtype=np.int32)

    def put(self, r, pos, x, w):
        raw, val = encode(x, self.split)
        s = np.asarray(pos) % self.cap
        self.raw[s, r], self.val[s, r], self.words[s, r] = raw, val, w


def launch(rg, pos0, nq, first, length, N, thetas, lpc_fill=FILL):
    dev = torch.device("cuda", torch.cuda.current_device())
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    hist, words = up(rg.raw, np.float32), up(rg.words, np.int32)
    fs, ln = up(first, np.int32), up(length, np.int32)
    lpc = torch.full((len(thetas), nq, rg.R), lpc_fill, device=dev, dtype=torch.float32)
    flags = torch.zeros(1, device=dev, dtype=torch.int32)
    th = (ctypes.c_float * len(thetas))(*[float(t) for t in thetas])
    torch.cuda.synchronize()
    rc = _lib.lib().jlm_cache_rows(hist.data_ptr(), words.data_ptr(), rg.cap, rg.R, rg.H, int(rg.split), H_SCALE, int(pos0), int(nq),
                                   fs.data_ptr(), ln.data_ptr(), int(N), th, len(thetas), lpc.data_ptr(), flags.data_ptr(), None)
    torch.cuda.synchronize()
    return rc, lpc.cpu().numpy(), int(flags.cpu()[0])


def reference(rg, pos0, nq, first, length, N, thetas):
    """-> (lpc [n_theta, nq, R] float64 with NaN where the row has no query, bar of the same shape) from the definition"""
    T = len(thetas)
    lpc = np.full((T, nq, rg.R), np.nan)
    bar = np.zeros((T, nq, rg.R))
    for r in range(rg.R):
        for q in range(min(int(length[r]), nq)):
            qp = pos0 + q
            idx = np.arange(max(qp - N, int(first[r]), 0), qp)
            lpc[:, q, r] = -np.inf
            if not len(idx):
                continue
            hq, hk = rg.val[qp % rg.cap, r], rg.val[idx % rg.cap, r]
            dot = hk @ hq
            A = float((np.abs(hk) @ np.abs(hq)).max())
            same = rg.words[idx % rg.cap, r] == rg.words[qp % rg.cap, r]
            if not same.any():
                continue
            for t, theta in enumerate(thetas):
                s = float(np.float32(theta)) * dot
                m = s.max()
                assert s[same].max() - m > -80.0                           # inside f32's exponent range (module docstring)
                logZ, logM = np.log(np.exp(s - m).sum()), np.log(np.exp(s[same] - m).sum())
                lpc[t, q, r] = logM - logZ
                bar[t, q, r] = kernel_bar(rg.split, rg.H, N, theta, A, logM, logZ)
    return lpc, bar


def check(rg, pos0, nq, first, length, N, thetas, tag):
    rc, got, flags = launch(rg, pos0, nq, first, length, N, thetas)
    assert rc == 0 and flags == 0, (tag, rc, flags)
    want, bar = reference(rg, pos0, nq, first, length, N, thetas)
    none = np.isnan(want)
    assert np.all(got[none] == np.float32(FILL)), tag                       # entries (q, r) with q >= len[r]: untouched
    minf = np.isneginf(want)
    assert np.array_equal(np.isneginf(got), minf) and not np.isnan(got).any(), tag            # no match: exactly -inf
    ok = ~none & ~minf
    err = np.abs(got[ok].astype(np.float64) - want[ok])
    worst = float((err / bar[ok]).max()) if ok.any() else 0.0
    print("%s: %d values, max |err| %.3e, max err / bar %.3f, max bar %.3e" % (tag, int(ok.sum()), err.max() if ok.any() else 0.0, worst,
                                                                              bar[ok].max() if ok.any() else 0.0))
    assert np.all(err <= bar[ok]), (tag, float(err.max()), worst)
    return got


def random_case(split, H, R, N, nq, carried, pos0, seed, ragged=True, n_words=5, cap=None):
    """rings with row r holding its ``carried[r % len]`` entries before pos0 and its len[r] queries from pos0 on; words from a small pool"""
    rng = np.random.RandomState(seed)
    rg = Rings(cap or N + nq, R, H, split)
    amp = min(0.999, 3.0 / H ** 0.25)                                      # h . h of a few units either way at every H
    length = np.sort(rng.randint(0, nq + 1, size=R))[::-1].copy() if ragged and R > 1 else np.full(R, nq)
    length[0] = nq
    first = np.zeros(R, dtype=np.int64)
    for r in range(R):
        k = min(carried[r % len(carried)], pos0)
        first[r] = pos0 - k
        pos = np.arange(first[r], pos0 + length[r])
        if len(pos):
            rg.put(r, pos, rng.uniform(-amp, amp, size=(len(pos), H)), rng.randint(0, n_words, size=len(pos)))
    return rg, first, length


# (split, H, R, N, nq, carried per row, n_theta): every value of each list at the smallest shape that reaches it.  H = 96 is three
# 32-blocks and no power of two; an H off the kernel's k-step (16 on split rows, 8 on f32 rows) does not exist: both LSTM steps take
# H % 32 == 0 only, and the launcher refuses what they refuse (test_refusals_on_the_device_library).
SHAPES = [
    (1, 64, 1, 1, 1, (0,), 1), (1, 64, 1, 1, 31, (1,), 1), (0, 64, 3, 3, 33, (0, 3), 3), (1, 64, 3, 3, 70, (3, 0, 2), 1),
    (1, 64, 3, 32, 33, (32, 5, 0), 3), (0, 64, 3, 32, 31, (5,), 1), (1, 64, 65, 33, 33, (33, 5, 0), 1), (0, 64, 65, 33, 1, (33, 0), 3),
    (1, 96, 3, 50, 70, (50, 5, 0), 3), (0, 96, 3, 50, 31, (0, 50), 1), (1, 512, 3, 50, 33, (50, 5), 1), (0, 512, 3, 33, 33, (5, 33), 3),
    (1, 512, 1, 32, 70, (0,), 3), (0, 512, 1, 50, 70, (50,), 1), (1, 64, 3, 4096, 70, (4096, 5, 0), 1), (0, 64, 1, 4096, 33, (4096,), 3),
    (1, 512, 65, 3, 31, (3, 0), 1), (1, 64, 1, 4096, 1, (4096,), 3),
]
THETAS = {1: [0.7], 3: [0.0, 0.3, 1.5]}


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%s-H%d-R%d-N%d-q%d-c%s-t%d" % (("f32", "split")[s[0]], s[1], s[2], s[3], s[4],
                                                                                      "_".join(map(str, s[5])), s[6]))
def test_shapes(shape):
    split, H, R, N, nq, carried, n_theta = shape
    seed = sum(shape[:5]) + 7 * n_theta
    cap = N + nq + seed % 3
    pos0 = 4 * cap - max(1, min(nq, N) // 2)                               # the window and the queries straddle the ring's end
    rg, first, length = random_case(split, H, R, N, nq, carried, pos0, seed, cap=cap)
    thetas = THETAS[n_theta]
    got = check(rg, pos0, nq, first, length, N, thetas, "shape %s" % (shape,))
    if n_theta > 1:                                                        # a theta's result does not depend on its neighbours
        for t, theta in enumerate(thetas):
            rc, one, fl = launch(rg, pos0, nq, first, length, N, [theta])
            assert rc == 0 and fl == 0 and one[0].tobytes() == got[t].tobytes(), (shape, theta)
    # positions numbered from the stream's start: the same entries before any wrap give the same window
    if max(carried) == 0:
        rg0, first0, length0 = random_case(split, H, R, N, nq, carried, 0, seed, cap=cap)
        check(rg0, 0, nq, first0, length0, N, thetas, "shape %s at pos0 = 0" % (shape,))


@pytest.mark.parametrize("split", [0, 1])
def test_theta_zero_counts_and_window_edges(split):
    """theta = 0: lpc = log(#matches / n_q) -- Z and M are exact integer sums in f32, so the error is logf's alone.  One matching entry
    moved across the window's old edge (q - N counts, q - N - 1 does not) and across ``first``"""
    H, R, N, nq = 64, 2, 37, 40
    cap = N + nq
    pos0 = 5 * cap - 9
    rng = np.random.RandomState(split)

    def run(match_pos, first):
        rg = Rings(cap, R, H, split)
        for r in range(R):
            pos = np.arange(pos0 - N - 2, pos0 + nq)
            rg.put(r, pos, rng.uniform(-1, 1, size=(len(pos), H)), 1000 + np.arange(len(pos)))       # every word its own
        q = pos0 + 20
        for r in range(R):
            rg.words[q % cap, r] = 7
            rg.words[match_pos % cap, r] = 7
        rc, got, fl = launch(rg, pos0, nq, first, [nq] * R, N, [0.0])
        assert rc == 0 and fl == 0
        assert np.all(np.isneginf(np.delete(got[0], 20, axis=0)))
        return got[0, 20]

    q = pos0 + 20
    tol = 5 * U * np.log(N) + 2 * U                   # logf twice, each within an ulp (<= 2 u |x|) of at most log N, and the subtraction
    assert np.all(np.abs(run(q - N, [0, 0]) - np.log(1.0 / N)) <= tol)
    assert np.all(np.isneginf(run(q - N - 1, [0, 0])))
    got = run(q - 5, [q - 5, q - 4])
    assert abs(got[0] - np.log(1.0 / 5)) <= tol and np.isneginf(got[1])
    # counts over a random match pattern, every query
    rg, first, length = random_case(split, H, 3, N, nq, (N, 5, 0), pos0, 99, n_words=3, cap=cap)
    rc, got, fl = launch(rg, pos0, nq, first, length, N, [0.0])
    assert rc == 0 and fl == 0
    for r in range(3):
        for qi in range(int(length[r])):
            qp = pos0 + qi
            idx = np.arange(max(qp - N, first[r]), qp)
            k = int(np.sum(rg.words[idx % cap, r] == rg.words[qp % cap, r])) if len(idx) else 0
            if k == 0:
                assert np.isneginf(got[0, qi, r])
            else:
                assert abs(got[0, qi, r] - np.log(k / len(idx))) <= tol, (r, qi, k, len(idx))


@pytest.mark.parametrize("split", [0, 1])
def test_every_entry_matching_and_peaked_scores(split):
    """every entry matching: M and Z are the same sums, lpc = 0.0 exactly (inside any bar).  Peaked scores: keys equal to the query,
    theta H in the hundreds -- every score is the same large number, which must stay finite with no flag: lpc = log(#matches / n_q)"""
    H, R, N, nq = 512, 2, 50, 33
    cap = N + nq
    pos0 = 2 * cap + 11
    rng = np.random.RandomState(5 + split)
    rg, first, length = random_case(split, H, R, N, nq, (N, 5), pos0, 17, ragged=False, n_words=1, cap=cap)
    got = check(rg, pos0, nq, first, length, N, [0.0, 0.9, 4.0], "all matching")
    has = np.zeros((nq, R), dtype=bool)
    for r in range(R):
        has[:, r] = (pos0 + np.arange(nq)) > first[r]
    assert np.all(got[:, has] == 0.0)
    # peaked: one vector of +-0.9 everywhere, h.h = 0.81 H = 414.72; theta = 0.8 -> s = 331.8 for every entry
    v = np.where(rng.rand(H) < 0.5, -0.9, 0.9)
    rg = Rings(cap, R, H, split)
    pos = np.arange(pos0 - N, pos0 + nq)
    for r in range(R):
        rg.put(r, pos, np.tile(v, (len(pos), 1)), rng.randint(0, 2, size=len(pos)))
    first = [pos0 - N] * R
    rc, got, fl = launch(rg, pos0, nq, first, [nq] * R, N, [0.8])
    assert rc == 0 and fl == 0 and np.isfinite(got[~np.isneginf(got)]).all() and not np.isnan(got).any()
    want, bar = reference(rg, pos0, nq, first, [nq] * R, N, [0.8])
    ok = np.isfinite(want)
    assert ok.any() and np.array_equal(np.isneginf(got), np.isneginf(want))
    assert np.all(np.abs(got[ok] - want[ok]) <= bar[ok])


@pytest.mark.parametrize("split", [0, 1])
def test_flag_and_untouched_rows(split):
    """a NaN planted in an existing entry sets flag 1; one planted in a slot outside every window does not; lpc of rows >= len stays"""
    H, R, N, nq = 64, 4, 20, 10
    cap = N + nq + 6
    pos0 = cap + 3
    rg, first, length = random_case(split, H, R, N, nq, (N,), pos0, 41, ragged=False, cap=cap)
    length = np.array([nq, 7, 0, 0])
    # slots outside every window: positions before pos0 - N are already NaN (Rings' fill) and rows 2, 3 have no query
    rg.raw[(pos0 + 1) % cap, 3] = NAN_BITS
    check(rg, pos0, nq, first, length, N, [0.5], "NaN outside every window")
    rc, got, fl = launch(rg, pos0, nq, first, length, N, [0.5])
    assert np.all(got[0, :, 2:] == np.float32(FILL)) and np.all(got[0, 7:, 1] == np.float32(FILL)) and fl == 0
    rg.raw[(pos0 - 3) % cap, 1, 5] = NAN_BITS                                 # an entry of row 1's windows
    rc, got2, fl = launch(rg, pos0, nq, first, length, N, [0.5])
    assert rc == 0 and fl == 1
    assert got2[0, :, 0].tobytes() == got[0, :, 0].tobytes()                  # the other rows are what they were


def test_refusals_on_the_device_library():
    """the launcher's -1 cases launch nothing (lpc untouched), empty shapes return 0"""
    rg, first, length = random_case(1, 64, 2, 8, 4, (8,), 12, 3, ragged=False)
    lib = _lib.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    hist = torch.from_numpy(rg.raw).to(dev)
    words = torch.from_numpy(rg.words).to(dev)
    fs = torch.tensor(first, dtype=torch.int32, device=dev)
    ln = torch.tensor(length, dtype=torch.int32, device=dev)
    lpc = torch.full((1, 4, 2), FILL, device=dev)
    th = (ctypes.c_float * 17)(*([0.5] * 17))
    neg = (ctypes.c_float * 1)(-1.0)
    base = [hist.data_ptr(), words.data_ptr(), rg.cap, 2, 64, 1, H_SCALE, 12, 4, fs.data_ptr(), ln.data_ptr(), 8, th, 1, lpc.data_ptr(), None, None]
    NAMES = ["hist", "words", "cap", "n_rows", "H", "split", "h_scale", "pos0", "n_query", "first", "len", "N", "thetas", "n_theta", "lpc"]

    def call(**kw):
        a = list(base)
        for k, v in kw.items():
            a[NAMES.index(k)] = v
        return lib.jlm_cache_rows(*a)

    for kw in (dict(cap=11), dict(H=0), dict(H=48), dict(hist=hist.data_ptr() + 4), dict(words=words.data_ptr() + 2), dict(lpc=None),
               dict(n_theta=0), dict(n_theta=17), dict(thetas=neg), dict(N=0), dict(pos0=-1), dict(h_scale=0.0), dict(n_rows=-1),
               dict(n_rows=65536)):
        assert call(**kw) == -1, kw
    assert call(n_rows=0) == 0 and call(n_query=0) == 0
    torch.cuda.synchronize()
    assert bool((lpc == FILL).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool((lpc == FILL).any())
