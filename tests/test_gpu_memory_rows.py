"""GPU: memory_rows_kernel / memory_fold_kernel as jlm_memory_rows launches them (csrc/jlm_memory.hip, include/jlm_hip.h), on keys and
query rows the test writes -- no model.  Every lpm is checked against the definition in float64 over the DECODED operands (split rows:
(hi + lo) / h_scale), within a bar that is derived here, not measured.

The bar.  u = 2^-24.  For a query q and an entry i, A_i = sum_k |q_k| |k_k| (real units).  The products, the scores and the online
update are cache_rows_kernel's instruction for instruction (tests/test_gpu_cache_rows.py), so their terms are that test's:

  products      split rows: three v_mfma_f32_32x32x16_f16 per 16 k into one f32 accumulator, every product of two f16 halves exact, an
                instruction's 16 products added with at most 2^-22 |C| of error, |C| <= (1 + 2^-10) A_i, 3 H / 16 instructions, the
                dropped lo.lo at most 2^-22 A_i:                              E_split(H) = (3 H / 16) 2^-22 (1 + 2^-9) + 2^-22
                f32 rows: v_mfma_f32_32x32x2_f32, a k-ordered fmaf chain of H terms:   E_f32(H) = H u / (1 - H u)
                (tests/cache_budget.py e_products, imported)
  scores        s_i = f32(theta' * dot) and the f32 difference s_i - m with |s_i - m| <= 2 theta max_i A_i add 3 u theta A:
                    |delta s_i| <= DS = theta * max_i A_i * (E(H) + 4 u)
  lpm           log sum exp is 1-Lipschitz in the largest |delta s_i|, once for log M and once for log Z:     2 DS
  the sums      M and Z are f32 sums of N positive terms: expf within 1 ulp (2 u relative) per term, N - 1 effective additions (u
                each, of positive partial sums; adding an empty partial sum is exact), and a partial sum is rescaled by
                expf(m_old - m_new) once per stage it passes (3 u: the expf and the product).  THIS kernel's stages: a wave reads the
                tile pairs w, w + 8, ... of ONE split -- ceil(min(S, N) / 32) tiles, S = keys per split -- so at most
                2 ceil(ceil(tiles / 2) / 8) tile stages; then the half-wave fold, the eight-wave fold of the workgroup (the two are the
                16-way fold) and the fold over the splits, one stage each:
                    ES = (2 + N + 3 (2 ceil(ceil(tiles / 2) / 8) + 3)) u * 1.01          on log M and on log Z each
  logf          within 1 ulp of its result, and the final f32 subtraction:   2 u (|log M| + |log Z|) + u |lpm|  (reference values,
                log Z and log M under the running maximum, + 2 u for results near 0)

  BAR_q = 2 DS + 2 ES + 2 u (|log M| + |log Z| + 1) + u |lpm|          (tests/memory_budget.py kernel_bar)

It holds while the largest matching term stays inside the f32 exponent range under the running maximum (s_match - m > -80: asserted
of every case's reference).  Exact values are asserted where the definition gives them: -inf without a match, 0.0 when every entry
matches (M and Z are then the same sums through every fold, bit for bit), entries of queries that are not live left untouched, and
a query's bits whatever else the launch carries.  Largest fraction of the bar seen: DESIGN.md section 28.
"""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
from jlm_amd import _lib                                                                  # noqa: E402
from tests import poison                                                                  # noqa: E402
from tests.memory_budget import U, kernel_bar, keys_per_split                              # noqa: E402
from tests.test_gpu_cache_rows import H_SCALE, NAN_BITS, encode                            # noqa: E402

pytestmark = pytest.mark.gpu

FILL = 123.0                                                                               # what lpm and its guards hold before a launch
GUARD = 64                                                                                 # floats of poison on either side of lpm
S512 = 512                                                                                 # keys per split at every N of this module
WORST = [0.0]


class Case:
    """keys [N, H] / key_words [N], queries [S, R, H] / q_words [S, R] with ``length`` [R] live steps a row; rows of queries that are
    not live hold NaN and the word -1 (never read)"""

    def __init__(self, split, H, N, R, S, seed, ragged=False, n_words=5, key_words=None, q_words=None):
        rng = np.random.RandomState(seed)
        amp = min(0.999, 3.0 / H ** 0.25)                                  # h . k of a few units either way at every H
        self.split, self.H, self.N, self.R, self.S = split, H, N, R, S
        self.k_raw, self.k_val = encode(rng.uniform(-amp, amp, size=(N, H)), split)
        self.q_raw, self.q_val = encode(rng.uniform(-amp, amp, size=(S, R, H)), split)
        self.k_words = np.asarray(rng.randint(0, n_words, size=N) if key_words is None else key_words, dtype=np.int32)
        self.q_words = np.asarray(rng.randint(0, n_words, size=(S, R)) if q_words is None else q_words, dtype=np.int32).reshape(S, R)
        self.length = np.full(R, S, dtype=np.int32)
        if ragged:
            self.length = np.sort(rng.randint(0, S + 1, size=R))[::-1].astype(np.int32)
            self.length[0] = S
            self.length[-1] = 0
        self.live = np.arange(S)[:, None] < self.length[None, :]
        self.q_raw[~self.live] = NAN_BITS
        self.q_words[~self.live] = -1


def launch(cs, values, ws_fill=None, use_len=True, flags=True, **over):
    """-> (rc, lpm [n_theta, S, R], the guards around it, flags)"""
    dev = torch.device("cuda", torch.cuda.current_device())
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    keys, kw, qr, qw, ln = up(cs.k_raw, np.float32), up(cs.k_words, np.int32), up(cs.q_raw, np.float32), up(cs.q_words, np.int32), up(cs.length, np.int32)
    n = len(values) * cs.S * cs.R
    buf = torch.full((GUARD + n + GUARD,), FILL, device=dev, dtype=torch.float32)
    lpm = buf[GUARD:GUARD + n]
    lib = _lib.lib()
    need = int(lib.jlm_memory_workspace_bytes(cs.N, cs.R, cs.S, len(values)))
    ws = torch.zeros(max(need // 4, 1), device=dev, dtype=torch.float32)
    if ws_fill is not None:
        poison.fill_tensor(ws, ws_fill)
    fl = torch.zeros(1, device=dev, dtype=torch.int32)
    th = (ctypes.c_float * len(values))(*[float(t) for t in values])
    a = dict(keys=keys.data_ptr(), key_words=kw.data_ptr(), N=cs.N, H=cs.H, split=int(cs.split), h_scale=H_SCALE, q_rows=qr.data_ptr(),
             q_words=qw.data_ptr(), n_rows=cs.R, n_steps=cs.S, len=ln.data_ptr() if use_len else None, thetas=th, n_theta=len(values),
             lpm=lpm.data_ptr(), workspace=ws.data_ptr(), workspace_bytes=need, flags=fl.data_ptr() if flags else None, stream=None)
    a.update(over)
    torch.cuda.synchronize()
    rc = lib.jlm_memory_rows(*a.values())
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    return rc, out[GUARD:GUARD + n].reshape(len(values), cs.S, cs.R).copy(), np.concatenate([out[:GUARD], out[GUARD + n:]]), int(fl.cpu()[0])


def reference(cs, thetas):
    """-> (lpm [n_theta, S, R] float64 with NaN where the query is not live, bar of the same shape) from the definition"""
    T = len(thetas)
    lpm = np.full((T, cs.S, cs.R), np.nan)
    bar = np.zeros((T, cs.S, cs.R))
    for t_, r in zip(*np.nonzero(cs.live)):
        hq = cs.q_val[t_, r]
        dot = cs.k_val @ hq
        A = float((np.abs(cs.k_val) @ np.abs(hq)).max())
        same = cs.k_words == cs.q_words[t_, r]
        lpm[:, t_, r] = -np.inf
        if not same.any():
            continue
        for t, theta in enumerate(thetas):
            s = float(np.float32(theta)) * dot
            m = s.max()
            assert s[same].max() - m > -80.0                               # inside f32's exponent range (module docstring)
            logZ, logM = np.log(np.exp(s - m).sum()), np.log(np.exp(s[same] - m).sum())
            lpm[t, t_, r] = logM - logZ
            bar[t, t_, r] = kernel_bar(cs.split, cs.H, cs.N, theta, A, logM, logZ)
    return lpm, bar


def check(cs, thetas, tag, **kw):
    rc, got, guards, flags = launch(cs, thetas, **kw)
    assert rc == 0 and flags == 0, (tag, rc, flags)
    assert np.all(guards == np.float32(FILL)), tag
    want, bar = reference(cs, thetas)
    none = np.isnan(want)
    assert np.all(got[none] == np.float32(FILL)), tag                       # queries that are not live: untouched
    minf = np.isneginf(want)
    assert np.array_equal(np.isneginf(got), minf) and not np.isnan(got).any(), tag            # no match: exactly -inf
    ok = ~none & ~minf
    err = np.abs(got[ok].astype(np.float64) - want[ok])
    worst = float((err / bar[ok]).max()) if ok.any() else 0.0
    WORST[0] = max(WORST[0], worst)
    print("%s: %d values, max |err| %.3e, max err / bar %.3f, max bar %.3e (largest fraction so far %.3f)" % (
        tag, int(ok.sum()), err.max() if ok.any() else 0.0, worst, bar[ok].max() if ok.any() else 0.0, WORST[0]))
    assert np.all(err <= bar[ok]), (tag, float(err.max()), worst)
    return got


# Both row formats x every N of the two lists -- {1, 31, 32, 33, 63, 64, 65}: the edges of a tile and of a tile pair; {S - 1, S, S + 1,
# 2 S + 33}, S = 512 = keys per split at these N: one split less a key, exactly one, a second split of one key, three splits with a
# ragged last one -- with H, the query shape (rows x steps) and the number of thetas cycling through their values, so that each value
# meets both formats and several splits.  An H off the kernel's k-step does not exist (H % 32 == 0, refused otherwise).
NS = [1, 31, 32, 33, 63, 64, 65, S512 - 1, S512, S512 + 1, 2 * S512 + 33]
HS = [64, 96, 512]
QUERIES = [(1, 1, False), (3, 11, False), (65, 1, False), (5, 13, True)]
THETAS = {1: [0.7], 3: [0.0, 0.3, 1.5]}
SHAPES = [(split, HS[(i + split) % 3], N, *QUERIES[(i + 2 * split) % 4], (1, 3)[(i + split) % 2]) for split in (0, 1) for i, N in enumerate(NS)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%s-H%d-N%d-R%d-S%d%s-t%d" % (("f32", "split")[s[0]], s[1], s[2], s[3], s[4],
                                                                                    "r" if s[5] else "", s[6]))
def test_shapes(shape):
    split, H, N, R, S, ragged, n_theta = shape
    assert keys_per_split(N) == S512 == _lib.lib().jlm_memory_keys_per_split(N)
    cs = Case(split, H, N, R, S, seed=N + 7 * H + R, ragged=ragged)
    thetas = THETAS[n_theta]
    got = check(cs, thetas, "shape %s" % (shape,))
    if n_theta > 1:                                                        # a theta's result does not depend on its neighbours
        for t, theta in enumerate(thetas):
            rc, one, _g, fl = launch(cs, [theta])
            assert rc == 0 and fl == 0 and one[0].tobytes() == got[t].tobytes(), (shape, theta)
    if not ragged:                                                         # len = NULL: every query live, the same bits
        rc, alln, _g, fl = launch(cs, thetas, use_len=False)
        assert rc == 0 and fl == 0 and alln.tobytes() == got.tobytes()


@pytest.mark.parametrize("split", [0, 1])
def test_exact_values_and_theta_zero_counts(split):
    """every entry matching: M and Z are the same sums through every fold, lpm = 0.0 exactly; no entry matching: -inf exactly;
    theta = 0 with m matches of N: log(m / N) within the bar (Z and M are exact integer sums in f32)"""
    H, N, R, S = 96, 2 * S512 + 33, 3, 11
    cs = Case(split, H, N, R, S, seed=5 + split, n_words=1)
    got = check(cs, [0.0, 0.9, 4.0], "all matching")
    assert np.all(got == 0.0)
    cs = Case(split, H, N, R, S, seed=6 + split, key_words=np.arange(N) + 10)
    rc, got, _g, fl = launch(cs, [0.0, 0.9])
    assert rc == 0 and fl == 0 and np.all(np.isneginf(got))
    # counts: word w is held by the entries i with i % 7 == w
    cs = Case(split, H, N, R, S, seed=8 + split, key_words=np.arange(N) % 7, q_words=np.arange(S * R) % 8)
    got = check(cs, [0.0], "theta 0")
    for t in range(S):
        for r in range(R):
            w = cs.q_words[t, r]
            m = int(np.sum(cs.k_words == w))
            if m == 0:
                assert w == 7 and np.isneginf(got[0, t, r])
            else:
                assert abs(got[0, t, r] - np.log(m / N)) <= 5 * U * np.log(N) + 2 * U     # logf twice, each within an ulp, and the subtraction
    # peaked scores: keys equal to the query, theta H in the hundreds -- every score the same large number, finite, no flag
    v = np.where(np.random.RandomState(1).rand(512) < 0.5, -0.9, 0.9)
    cs = Case(split, 512, S512 + 1, 2, 3, seed=9, n_words=2)
    cs.k_raw, cs.k_val = encode(np.tile(v, (cs.N, 1)), split)
    cs.q_raw, cs.q_val = encode(np.tile(v, (3, 2, 1)), split)
    check(cs, [0.8], "peaked")


@pytest.mark.parametrize("split", [0, 1])
def test_workspace_content_and_repeat(split):
    """the same bits whether the workspace held zeros, NaN or 1e30 before the call (tests/poison.py's fills), and on a second run"""
    cs = Case(split, 64, 2 * S512 + 33, 5, 13, seed=21, ragged=True)
    thetas = THETAS[3]
    base = check(cs, thetas, "workspace zeroed")
    for fill in poison.FILLS:
        rc, got, guards, fl = launch(cs, thetas, ws_fill=fill)
        assert rc == 0 and fl == 0 and np.all(guards == np.float32(FILL))
        assert poison.bits(got) == poison.bits(base), (fill.name, poison.first_difference(got, base, "lpm"))
    rc, again, _g, fl = launch(cs, thetas)
    assert poison.bits(again) == poison.bits(base)


@pytest.mark.parametrize("split", [0, 1])
def test_a_querys_bits_do_not_depend_on_the_launch(split):
    """one query launched alone, among 65 queries (another column, another block), among queries of which most are not live, and
    with 1 or 3 thetas: the same bits"""
    H, N = 64, 2 * S512 + 33
    big = Case(split, H, N, 65, 1, seed=33)
    thetas = THETAS[3]
    got = check(big, thetas, "65 queries")
    for r in (0, 31, 32, 64):
        one = Case(split, H, N, 1, 1, seed=33)
        one.k_raw, one.k_val, one.k_words = big.k_raw, big.k_val, big.k_words
        one.q_raw, one.q_val, one.q_words = big.q_raw[:, r:r + 1].copy(), big.q_val[:, r:r + 1], big.q_words[:, r:r + 1].copy()
        rc, alone, _g, fl = launch(one, thetas)
        assert rc == 0 and fl == 0 and alone[:, 0, 0].tobytes() == got[:, 0, r].tobytes(), r
        rc, alone1, _g, fl = launch(one, thetas[1:2])
        assert rc == 0 and alone1[0, 0, 0].tobytes() == got[1, 0, r].tobytes(), r
    # the same 65 rows as 5 steps of 13 rows with ragged lengths: a live query keeps its bits where it now stands
    rag = Case(split, H, N, 13, 5, seed=33, ragged=True)
    rag.k_raw, rag.k_val, rag.k_words = big.k_raw, big.k_val, big.k_words
    rag.q_raw, rag.q_val = big.q_raw.reshape(5, 13, -1).copy(), big.q_val.reshape(5, 13, -1)
    rag.q_words = big.q_words.reshape(5, 13).copy()
    rag.q_raw[~rag.live] = NAN_BITS
    rc, part, _g, fl = launch(rag, thetas)
    assert rc == 0 and fl == 0
    whole = got.reshape(3, 5, 13)
    assert rag.live.sum() > 13 and np.array_equal(part[:, rag.live].view(np.uint32), whole[:, rag.live].view(np.uint32))
    assert np.all(part[:, ~rag.live] == np.float32(FILL))


@pytest.mark.parametrize("split", [0, 1])
def test_flag(split):
    """a NaN planted in a key sets flag bit 0; an unflagged launch leaves the flag at 0; a NULL flag pointer is accepted"""
    cs = Case(split, 64, S512 + 1, 3, 4, seed=41)
    rc, got, _g, fl = launch(cs, [0.5])
    assert rc == 0 and fl == 0
    cs.k_raw[S512, 5] = NAN_BITS                                              # the one key of the second split
    rc, _got2, _g, fl = launch(cs, [0.5])
    assert rc == 0 and fl == 1
    rc, _got3, guards, fl = launch(cs, [0.5], flags=False)
    assert rc == 0 and fl == 0 and np.all(guards == np.float32(FILL))


def test_refusals_on_the_device_library():
    """the launcher's -1 cases launch nothing (lpm untouched), empty shapes return 0"""
    cs = Case(1, 64, 40, 2, 4, seed=3)
    need = int(_lib.lib().jlm_memory_workspace_bytes(cs.N, cs.R, cs.S, 1))
    th17 = (ctypes.c_float * 17)(*([0.5] * 17))
    neg = (ctypes.c_float * 1)(-1.0)
    inf = (ctypes.c_float * 1)(float("inf"))
    probe = launch(cs, [0.5])
    assert probe[0] == 0 and not np.any(probe[1] == np.float32(FILL))

    def refused(**kw):
        rc, got, guards, fl = launch(cs, [0.5], **kw)
        assert np.all(got == np.float32(FILL)) and np.all(guards == np.float32(FILL)) and fl == 0, kw
        return rc

    for kw in (dict(N=0), dict(N=-5), dict(N=(1 << 24) + 1), dict(H=0), dict(H=48), dict(keys=None), dict(key_words=None), dict(q_rows=None),
               dict(q_words=None), dict(lpm=None), dict(workspace=None), dict(n_theta=0), dict(n_theta=17, thetas=th17), dict(thetas=None),
               dict(thetas=neg), dict(thetas=inf), dict(h_scale=0.0), dict(h_scale=-2.0), dict(n_rows=-1), dict(n_steps=-1),
               dict(n_rows=65536), dict(workspace_bytes=need - 4), dict(workspace_bytes=0)):
        assert refused(**kw) == -1, kw
    dev = torch.device("cuda", torch.cuda.current_device())
    odd = torch.zeros(cs.N * cs.H + 64, device=dev, dtype=torch.float32)
    for kw in (dict(keys=odd.data_ptr() + 4), dict(q_rows=odd.data_ptr() + 8), dict(key_words=odd.data_ptr() + 2),
               dict(q_words=odd.data_ptr() + 1), dict(workspace=odd.data_ptr() + 2), dict(len=odd.data_ptr() + 2)):
        assert refused(**kw) == -1, kw
    assert refused(n_rows=0) == 0 and refused(n_steps=0) == 0
