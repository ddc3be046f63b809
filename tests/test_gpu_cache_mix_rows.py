"""GPU: cache_query_kernel and cache_mix_rows_kernel as jlm_cache_query / jlm_cache_mix_rows launch them (csrc/jlm_cache_mix.hip,
include/jlm_hip.h), on rings, queries and logits the test writes -- no model.  Every s, every lpc_ent and every patched logit is
checked against the definition in float64 over the DECODED operands (split rows: (hi + lo) / h_scale), within the bars of
tests/cache_mix_budget.py, whose docstring holds the derivation term by term; nothing there is measured, and each test prints its
measured maximum as a share of the bar.  Exact values are asserted where the definition gives them: every word outside the window
keeps its bits, a repeat's lpc_ent is -inf, rows that are not live, empty windows and lambda = 0 leave every byte, a row gives the
same bits alone as among seventeen and at another pos / cap, and two launches give the same bits."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
from jlm_amd import _lib                                                                  # noqa: E402
from jlm_amd.cache import mixed_logits                                                    # noqa: E402
from tests.cache_mix_budget import U, lpc_bar, lse_bar, score_bar, y_bar                  # noqa: E402
from tests.row_lse_pin import CASES as LSE_CASES, LAM as LSE_LAM, expected_bits, pin_row  # noqa: E402
from tests.test_gpu_cache_rows import H_SCALE, NAN_BITS, Rings, encode                    # noqa: E402

pytestmark = pytest.mark.gpu

FILL = 123.0                                                                               # what s and lpc_ent hold before a launch


class Case:
    """One launch pair: rings [cap][n_rows][H] / [cap][n_rows] holding row r's window of lens[r] <= N entries before ``pos`` (NaN / -1
    everywhere else), the queries, logits y [n_rows, ld_y] with NaN in the padding, and the launch's scalars."""

    def __init__(self, split, H, R, N, V, lens, words, seed, pos=None, cap=None, self_norm=0, theta=0.7, lam=0.2, live=None, n_dev=None):
        rng = np.random.RandomState(seed)
        self.split, self.H, self.R, self.N, self.V = split, H, R, N, V
        self.self_norm, self.theta, self.lam = self_norm, theta, lam
        self.cap = cap or N + seed % 3
        self.pos = 3 * self.cap + max(1, N // 2) if pos is None else pos                   # the window straddles the ring's end
        self.live, self.n_dev = R if live is None else live, n_dev
        self.rg = Rings(self.cap, R, H, split)
        self.first = np.zeros(R, dtype=np.int64)
        amp = min(0.999, 3.0 / H ** 0.25)                                                  # h . h of a few units either way at every H
        self.lens = [min(int(lens[r % len(lens)]), N, self.pos) for r in range(R)]
        for r in range(R):
            n = self.lens[r]
            # a window shorter than N is cut by `first`; a full one has its first position anywhere at or before pos - N
            self.first[r] = self.pos - n if n < N else max(self.pos - N - (r % 2) * 5, 0)
            if n:
                p = np.arange(self.pos - n, self.pos)
                self.rg.put(r, p, rng.uniform(-amp, amp, size=(n, H)), words(rng, n, r))
        self.q_raw, self.q_val = encode(rng.uniform(-amp, amp, size=(R, H)), split)
        self.ld_y = (V + 3) // 4 * 4 + 4
        self.y = np.full((R, self.ld_y), NAN_BITS, dtype=np.float32)
        self.y[:, :V] = (3.0 * rng.standard_normal((R, V))).astype(np.float32)

    def n_live(self):
        return min(self.live, self.R if self.n_dev is None else self.n_dev)

    def window(self, r):
        """(positions, float64 keys [n, H], words [n]) of row r, oldest first"""
        idx = np.arange(max(self.pos - self.N, int(self.first[r]), 0), self.pos)
        return idx, self.rg.val[idx % self.cap, r], self.rg.words[idx % self.cap, r]


def pool(ids):
    return lambda rng, n, r: rng.choice(np.asarray(ids), size=n)


def equal(w):
    return lambda rng, n, r: np.full(n, w)


def distinct(V):
    return lambda rng, n, r: rng.permutation(V)[:n]


def paired(V):
    """w_j = ((j + 1) // 2) % V: entries 2 k - 1 and 2 k share a word, so a repeat straddles every even boundary of the window index"""
    return lambda rng, n, r: ((np.arange(n) + 1) // 2) % V


def launch(cs, y=None, mix=True, lpc_ent=True):
    """-> (rc_query, rc_mix, s [R, ld_s], y' [R, ld_y], lpc_ent [R, ld_s], flags)"""
    dev = torch.device("cuda", torch.cuda.current_device())
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    hist, words, q, first = up(cs.rg.raw, np.float32), up(cs.rg.words, np.int32), up(cs.q_raw, np.float32), up(cs.first, np.int32)
    yd = up(cs.y if y is None else y, np.float32)
    ld_s = cs.N + 3
    s = torch.full((cs.R, ld_s), FILL, device=dev, dtype=torch.float32)
    ent = torch.full((cs.R, ld_s), FILL, device=dev, dtype=torch.float32)
    flags = torch.zeros(1, device=dev, dtype=torch.int32)
    nd = torch.tensor([cs.n_dev], device=dev, dtype=torch.int32) if cs.n_dev is not None else None
    lib = _lib.lib()
    torch.cuda.synchronize()
    rc_q = lib.jlm_cache_query(hist.data_ptr(), cs.cap, cs.R, cs.H, int(cs.split), H_SCALE, q.data_ptr(), cs.live,
                               nd.data_ptr() if nd is not None else None, cs.pos, first.data_ptr(), cs.N, cs.theta, s.data_ptr(), ld_s,
                               flags.data_ptr(), None)
    rc_m = None
    if mix and rc_q == 0:
        rc_m = lib.jlm_cache_mix_rows(yd.data_ptr(), cs.ld_y, cs.V, cs.self_norm, s.data_ptr(), ld_s, words.data_ptr(), cs.cap, cs.R, cs.live,
                                      nd.data_ptr() if nd is not None else None, cs.pos, first.data_ptr(), cs.N, cs.lam,
                                      ent.data_ptr() if lpc_ent else None, flags.data_ptr(), None)
    torch.cuda.synchronize()
    return rc_q, rc_m, s.cpu().numpy(), yd.cpu().numpy(), ent.cpu().numpy(), int(flags.cpu()[0])


def same_bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def check(cs, tag, want_flags=0):
    """both launches against the definition; -> (s, y', lpc_ent)"""
    rc_q, rc_m, s, y2, ent, flags = launch(cs)
    assert rc_q == 0 and rc_m == 0 and flags == want_flags, (tag, rc_q, rc_m, flags)
    th = float(np.float32(cs.theta))
    log_rho = np.log(np.float32(cs.lam).astype(np.float64)) - np.log1p(-np.float32(cs.lam).astype(np.float64))
    worst = {"s": 0.0, "lpc": 0.0, "y": 0.0}
    n_val = 0
    for r in range(cs.R):
        idx, keys, ww = cs.window(r)
        n = len(idx)
        if r >= cs.n_live() or n == 0:                                     # not live, or an empty window: every byte as it was
            assert np.all(s[r] == np.float32(FILL)) and np.all(ent[r] == np.float32(FILL)) and same_bits(y2[r], cs.y[r]), (tag, r)
            continue
        assert np.all(s[r, n:] == np.float32(FILL)) and np.all(ent[r, n:] == np.float32(FILL)), (tag, r)
        dot = keys @ cs.q_val[r]
        A = float((np.abs(keys) @ np.abs(cs.q_val[r])).max())
        err_s = np.abs(s[r, :n].astype(np.float64) - th * dot)
        s_b = score_bar(cs.split, cs.H, cs.theta, A)
        if s_b > 0:
            worst["s"] = max(worst["s"], float(err_s.max()) / s_b)
        assert np.all(err_s <= s_b), (tag, r, float(err_s.max()), s_b)
        # the definition, in float64: c over every word; the out-of-range words of a window count in Z only
        sc = th * dot
        e = np.exp(sc - sc.max())
        logZ = np.log(e.sum())
        valid = (ww >= 0) & (ww < cs.V)
        c = np.zeros(cs.V)
        np.add.at(c, ww[valid], e[valid] / e.sum())
        yr = cs.y[r, :cs.V].astype(np.float64)
        want_y = mixed_logits(yr, c, float(np.float32(cs.lam)), bool(cs.self_norm))
        L = 0.0 if cs.self_norm else yr.max() + np.log(np.exp(yr - yr.max()).sum())
        L_b = lse_bar(yr, cs.self_norm)
        seen = set()
        touched = np.zeros(cs.ld_y, dtype=bool)
        for j in range(n):
            w = int(ww[j])
            if w in seen:
                assert np.isneginf(ent[r, j]), (tag, r, j)                 # a repeat
                continue
            seen.add(w)
            logc = np.log(e[ww == w].sum())
            assert logc > -80.0                                            # inside f32's exponent range under the maximum
            b = lpc_bar(cs.split, cs.H, cs.N, cs.theta, A, logc, logZ)
            err = abs(float(ent[r, j]) - (logc - logZ))
            worst["lpc"] = max(worst["lpc"], err / b)
            assert err <= b, (tag, r, j, err, b)
            if not valid[j]:
                continue
            touched[w] = True
            yb = y_bar(b, L_b, L, log_rho, logc - logZ, yr[w], want_y[w])
            err = abs(float(y2[r, w]) - want_y[w])
            worst["y"] = max(worst["y"], err / yb)
            assert err <= yb, (tag, r, j, w, err, yb)
            n_val += 1
        assert same_bits(y2[r][~touched], cs.y[r][~touched]), (tag, r)     # every other word, and the padding: the same bits
    print("%s: %d patched words, max err / bar: s %.3f, lpc_ent %.3f, y' %.3f" % (tag, n_val, worst["s"], worst["lpc"], worst["y"]))
    return s, y2, ent


# (split, H, R, live, n_dev, N, V, self_norm, window lengths per row, words, theta): every value of each list of the issue at the
# smallest shape that reaches it.  N = 31 / 32 / 33: the wave's edge in the mix kernel's tree; 255 / 256 / 257: its workgroup's, and
# the query kernel's chunks of 64 keys; 4096 = JLM_CACHE_MIX_MAX_N.  V = 5: a vocabulary inside one 16-byte chunk; 2 003: odd, three
# waves' worth of chunks.  lens: 10 ** 6 = a full window.
FULL = 10 ** 6
SHAPES = [
    (1, 32, 1, 1, None, 1, 5, 0, (FULL,), pool([0, 4]), 0.7),
    (0, 32, 1, 1, None, 2, 5, 1, (FULL,), pool([0, 1, 4]), 0.7),
    (1, 64, 3, 3, 2, 31, 2003, 0, (FULL, 7, 0), pool([0, 2002, 17, 18, 900]), 0.7),
    (0, 64, 3, 3, None, 32, 2003, 1, (FULL, 31, 1), paired(2003), 2.0),
    (1, 96, 3, 3, None, 33, 5, 0, (FULL, 32, 0), pool([0, 1, 2, 3, 4]), 0.5),
    (0, 96, 17, 17, 11, 255, 2003, 0, (FULL, 64, 65, 0, 200), paired(2003), 0.7),
    (1, 512, 3, 3, None, 256, 2003, 0, (FULL, 129), distinct(2003), 0.3),
    (0, 512, 3, 2, None, 257, 2003, 1, (FULL, 256), pool([0, 2002, 5]), 0.3),
    (1, 64, 17, 17, 16, 257, 5, 1, (FULL, 255, 3), equal(4), 2.0),
    (0, 64, 1, 1, None, 4096, 2003, 0, (FULL,), paired(2003), 0.7),
    (1, 64, 3, 3, 2, 4096, 2003, 0, (4095, FULL), pool(list(range(0, 2003, 167)) + [2002]), 0.7),
    (1, 96, 1, 1, None, 4096, 5, 1, (FULL,), equal(0), 0.5),
]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%s-H%d-R%d_%d_%s-N%d-V%d-sn%d" % (("f32", "split")[s[0]], s[1], s[2], s[3], s[4],
                                                                                          s[5], s[6], s[7]))
def test_shapes(shape):
    split, H, R, live, n_dev, N, V, self_norm, lens, words, theta = shape
    seed = split + H + R + N + V
    cs = Case(split, H, R, N, V, lens, words, seed, self_norm=self_norm, theta=theta, live=live, n_dev=n_dev)
    s, y2, ent = check(cs, "shape %s" % (shape[:8],))
    # two launches on the same inputs: the same bits
    _, _, s_b, y_b, ent_b, _ = launch(cs)
    assert same_bits(s, s_b) and same_bits(y2, y_b) and same_bits(ent, ent_b)
    # without the optional output the logits are the same bits
    _, _, _, y_c, ent_c, _ = launch(cs, lpc_ent=False)
    assert same_bits(y2, y_c) and np.all(ent_c == np.float32(FILL))


@pytest.mark.parametrize("split", [0, 1])
def test_theta_zero_is_a_count_share(split):
    """theta = 0: every s is 0.0 exactly, e = 1, c(w) Z = the number of entries holding w and Z = n_q, exact integers in f32: lpc_ent is
    log(count / n_q) within logf's error alone"""
    N, V = 97, 2003
    cs = Case(split, 64, 3, N, V, (FULL, 40, 1), pool([0, 5, 2002]), 11 + split, theta=0.0)
    s, y2, ent = check(cs, "theta = 0")
    tol = 5 * U * np.log(N) + 2 * U                                        # logf twice, each within an ulp, and the subtraction
    for r in range(3):
        idx, _, ww = cs.window(r)
        assert np.all(s[r, :len(idx)] == 0.0)
        seen = set()
        for j, w in enumerate(ww):
            if w not in seen:
                seen.add(w)
                assert abs(ent[r, j] - np.log(np.sum(ww == w) / len(ww))) <= tol, (r, j)


@pytest.mark.parametrize("self_norm", [0, 1])
def test_lambda_zero_and_no_window_leave_every_byte(self_norm):
    cs = Case(1, 64, 3, 33, 2003, (FULL, 5, 9), pool([0, 7, 2002]), 5, self_norm=self_norm, lam=0.0)
    rc_q, rc_m, s, y2, ent, flags = launch(cs)
    assert rc_q == 0 and rc_m == 0 and flags == 0
    assert same_bits(y2, cs.y) and np.all(ent == np.float32(FILL))         # lambda = 0 launches nothing
    cs = Case(0, 64, 3, 33, 2003, (0,), pool([0, 7, 2002]), 6, self_norm=self_norm)
    rc_q, rc_m, s, y2, ent, flags = launch(cs)
    assert rc_q == 0 and rc_m == 0 and flags == 0
    assert same_bits(y2, cs.y) and np.all(ent == np.float32(FILL)) and np.all(s == np.float32(FILL))
    # a stream's first position: pos = 0, first = 0
    cs = Case(0, 64, 2, 33, 2003, (FULL,), pool([0, 7]), 7, self_norm=self_norm, pos=0)
    rc_q, rc_m, s, y2, ent, flags = launch(cs)
    assert rc_q == 0 and rc_m == 0 and flags == 0 and same_bits(y2, cs.y) and np.all(s == np.float32(FILL))


@pytest.mark.parametrize("self_norm", [0, 1])
def test_a_cached_word_the_model_gives_no_mass(self_norm):
    """y[w] = -inf with c(w) > 0: y'[w] is the finite cache term L + log rho + log c(w)"""
    cs = Case(1, 64, 2, 40, 2003, (FULL, 9), pool([3, 700, 2002]), 21, self_norm=self_norm)
    cs.y[:, 700] = -np.inf
    cs.y[:, 1] = -np.inf                                                   # not in any window: stays -inf
    _, y2, _ = check(cs, "y[w] = -inf")
    for r in range(2):
        assert (700 in cs.window(r)[2]) == bool(np.isfinite(y2[r, 700]))
        assert np.isneginf(y2[r, 1])
    assert np.isfinite(y2[0, 700])


@pytest.mark.parametrize("V,where", LSE_CASES)
def test_L_is_the_topk_kernels_log_normaliser_bit_for_bit(V, where):
    """tests/row_lse_pin.py: one live row whose maximum 0.0f sits in the first or the last non-empty wave span, a window of exactly one
    entry holding w* (e = 1, Z = 1, c = 1 whatever the score) and y[w*] = -inf -- y'[w*] has the bits of
    float32(float32(nll) + log rho), nll jlm_topk_rows' own"""
    y, p, ws = pin_row(V, where)
    cs = Case(0, 32, 1, 1, V, (FULL,), equal(ws), 1, lam=LSE_LAM)
    assert cs.window(0)[2].tolist() == [ws]
    cs.y[0, :V] = y
    rc_q, rc_m, _, y2, ent, flags = launch(cs)
    assert rc_q == 0 and rc_m == 0 and flags == 0, (rc_q, rc_m, flags)
    assert ent[0, 0] == 0.0                                                # log c - log Z of the one entry
    got, want = int(y2[0, ws:ws + 1].view(np.uint32)[0]), expected_bits(V, where)
    print("V %d, p = %d (%s span), w* = %d: y'[w*] bits %08x, float32(float32(nll) + log rho) bits %08x" % (V, p, where, ws, got, want))
    assert got == want, (V, where, hex(got), hex(want))
    keep = np.ones(cs.ld_y, dtype=bool)
    keep[ws] = False
    assert same_bits(y2[0][keep], cs.y[0][keep])


def test_flags_leave_the_row_unpatched():
    """a NaN state: bit 1, the row as it was; a +inf logit (L not finite): bit 2, the row as it was; an out-of-range word: bit 4, the
    entry counts in Z (check() holds the other words to the definition with it) and nothing is indexed by it; the other rows of each
    launch are the bits of a clean launch"""
    mk = lambda: Case(1, 64, 4, 37, 2003, (FULL, 20, 36, 5), pool([0, 11, 2002]), 31)
    _, clean, _ = check(mk(), "clean")
    cs = mk()
    cs.rg.raw[(cs.pos - 3) % cs.cap, 1, 5] = NAN_BITS                       # an entry of row 1's window
    rc_q, rc_m, s, y2, ent, flags = launch(cs)
    assert rc_q == 0 and rc_m == 0 and flags == 1
    assert same_bits(y2[1], cs.y[1]) and np.all(ent[1] == np.float32(FILL))
    assert same_bits(np.delete(y2, 1, axis=0), np.delete(clean, 1, axis=0))
    cs = mk()
    cs.q_raw[2, 0] = NAN_BITS                                              # row 2's query
    rc_q, rc_m, s, y2, ent, flags = launch(cs)
    assert flags == 1 and same_bits(y2[2], cs.y[2]) and same_bits(np.delete(y2, 2, axis=0), np.delete(clean, 2, axis=0))
    cs = mk()
    cs.y[0, 9] = np.inf
    rc_q, rc_m, s, y2, ent, flags = launch(cs)
    assert rc_q == 0 and rc_m == 0 and flags == 2
    assert same_bits(y2[0], cs.y[0]) and same_bits(y2[1:], clean[1:])
    for bad in (-1, 2003, 1 << 30):
        cs = mk()
        cs.rg.words[(cs.pos - 2) % cs.cap, 3] = bad
        cs.rg.words[(cs.pos - 4) % cs.cap, 3] = bad
        _, y2, _ = check(cs, "word %d in a window" % bad, want_flags=4)
        assert same_bits(y2[:3], clean[:3])


@pytest.mark.parametrize("split", [0, 1])
def test_a_row_alone_among_seventeen_and_at_another_position(split):
    """y', s and lpc_ent of a row are functions of its window, its query, its logits and (theta, lambda): the same bits alone as among
    seventeen rows, and with the window at another pos / cap, wrapped round the ring's end or not, cut by `first` or by N"""
    H, N, V, n = 96, 70, 2003, 70
    base = Case(split, H, 17, N, V, (FULL, 33, 1), paired(V), 3, cap=N + 2)
    s17, y17, e17 = check(base, "seventeen rows")
    for r in (0, 1, 16):
        idx, _, ww = base.window(r)
        k = len(idx)
        for pos, cap in ((k, 4 * N), (5 * (N + 9) + 3, N + 9), (2 * N, N)):
            one = Case(split, H, 1, N, V, (k,), paired(V), 3, cap=cap, pos=pos)
            src = idx % base.cap
            dst = np.arange(pos - k, pos) % cap
            one.rg.raw[dst, 0], one.rg.val[dst, 0], one.rg.words[dst, 0] = base.rg.raw[src, r], base.rg.val[src, r], base.rg.words[src, r]
            one.first[0] = pos - k if r != 0 else max(pos - N - 1, 0)
            one.q_raw[0], one.q_val[0], one.y[0] = base.q_raw[r], base.q_val[r], base.y[r]
            rc_q, rc_m, s1, y1, e1, flags = launch(one)
            assert rc_q == 0 and rc_m == 0 and flags == 0
            assert same_bits(s1[0], s17[r]) and same_bits(y1[0], y17[r]) and same_bits(e1[0], e17[r]), (r, pos, cap)


def test_refusals_on_the_device_library():
    """every -1 of the two launchers launches nothing (s, y, lpc_ent untouched); empty shapes return 0"""
    cs = Case(1, 64, 2, 8, 2003, (FULL,), pool([0, 7]), 3)
    dev = torch.device("cuda", torch.cuda.current_device())
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    hist, words, q, first = up(cs.rg.raw, np.float32), up(cs.rg.words, np.int32), up(cs.q_raw, np.float32), up(cs.first, np.int32)
    y = up(cs.y, np.float32)
    s = torch.full((2, 8), FILL, device=dev)
    ent = torch.full((2, 8), FILL, device=dev)
    lib = _lib.lib()
    QN = ["hist", "cap", "n_rows", "H", "split", "h_scale", "q_rows", "n_rows_max", "n_dev", "pos", "first", "N", "theta", "s", "ld_s", "flags"]
    qbase = [hist.data_ptr(), cs.cap, 2, 64, 1, H_SCALE, q.data_ptr(), 2, None, cs.pos, first.data_ptr(), 8, 0.5, s.data_ptr(), 8, None, None]
    MN = ["y", "ld_y", "n_cols", "self_norm", "s", "ld_s", "words", "cap", "n_rows", "n_rows_max", "n_dev", "pos", "first", "N", "lam",
          "lpc_ent", "flags"]
    mbase = [y.data_ptr(), cs.ld_y, cs.V, 0, s.data_ptr(), 8, words.data_ptr(), cs.cap, 2, 2, None, cs.pos, first.data_ptr(), 8, 0.2,
             ent.data_ptr(), None, None]

    def call(fn, names, base, **kw):
        a = list(base)
        for k, v in kw.items():
            a[names.index(k)] = v
        return fn(*a)

    cq = lambda **kw: call(lib.jlm_cache_query, QN, qbase, **kw)
    cm = lambda **kw: call(lib.jlm_cache_mix_rows, MN, mbase, **kw)
    for kw in (dict(N=0), dict(N=4097, ld_s=4097, cap=4097), dict(cap=7), dict(ld_s=7), dict(H=0), dict(H=48), dict(theta=-1.0),
               dict(theta=float("inf")), dict(theta=float("nan")), dict(h_scale=0.0), dict(pos=-1), dict(pos=0x7fffffff - 3),
               dict(n_rows_max=3), dict(n_rows_max=-1), dict(n_rows=-1), dict(hist=hist.data_ptr() + 4), dict(q_rows=q.data_ptr() + 8),
               dict(hist=None), dict(q_rows=None), dict(s=None), dict(first=None), dict(s=s.data_ptr() + 2),
               dict(flags=s.data_ptr() + 1), dict(n_dev=s.data_ptr() + 2)):
        assert cq(**kw) == -1, kw
    for kw in (dict(N=0), dict(N=4097, ld_s=4097, cap=4097), dict(cap=7), dict(ld_s=7), dict(lam=-0.1), dict(lam=1.0), dict(lam=float("nan")),
               dict(pos=-1), dict(n_rows_max=3), dict(n_cols=0), dict(ld_y=cs.ld_y + 1), dict(ld_y=2000), dict(y=y.data_ptr() + 4),
               dict(y=None), dict(s=None), dict(words=None), dict(first=None), dict(words=words.data_ptr() + 2),
               dict(lpc_ent=ent.data_ptr() + 1), dict(lam=-0.1, n_rows_max=0)):
        assert cm(**kw) == -1, kw
    assert cq(n_rows_max=0) == 0 and cm(n_rows_max=0) == 0 and cm(lam=0.0) == 0
    torch.cuda.synchronize()
    assert bool((s == FILL).all()) and bool((ent == FILL).all()) and same_bits(y.cpu().numpy(), cs.y)
    assert cq() == 0 and cm() == 0
    torch.cuda.synchronize()
    assert not bool((s == FILL).any()) and not same_bits(y.cpu().numpy(), cs.y)
