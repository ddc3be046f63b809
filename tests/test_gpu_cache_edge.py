"""GPU: cache_cell_query_kernel and cache_cell_patch_kernel as jlm_cache_cell_query / jlm_cache_cell_patch launch them
(csrc/jlm_cache_edge.hip, include/jlm_hip.h), on windows, queries, word lists and slices the test writes -- no model.

Query: every s is bit-equal to jlm_cache_query's for the same (query row, key row, theta), within cache_mix_budget.score_bar of the
float64 product over the DECODED operands, and gives the same bits alone as among other cells; nothing outside the live slots and the
window is written.  Patch: every rewritten edge logit within decode_cache_budget.edge_bar of the float64 definition (each test prints
its measured share of the bar), the edge rows of a sentence without a window bit-unchanged, the folded log-normalisers bit-equal to
what jlm_beam_step's fused fold writes from the same slices, and a log-normaliser that is not finite flagged and replaced."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
from jlm_amd import _lib                                                                  # noqa: E402
from tests.cache_mix_budget import U, score_bar                                           # noqa: E402
from tests.decode_cache_budget import edge_bar                                            # noqa: E402
from tests.test_gpu_cache_rows import H_SCALE, NAN_BITS, encode                           # noqa: E402

pytestmark = pytest.mark.gpu

FILL = 123.0
THETA = 0.7


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def up(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev())


class Window:
    """cache rows [cap][n_src]: row r's count[r] entries in the slots cap - count[r] .. cap - 1, NaN / -1 below"""

    def __init__(self, split, H, cap, counts, seed, words=None):
        rng = np.random.RandomState(seed)
        self.split, self.H, self.cap, self.count = split, H, cap, np.asarray(counts, dtype=np.int32)
        n_src = len(counts)
        self.raw = np.full((cap, n_src, H), NAN_BITS, dtype=np.float32)
        self.val = np.full((cap, n_src, H), np.nan)
        self.words = np.full((cap, n_src), -1, dtype=np.int32)
        amp = min(0.999, 3.0 / H ** 0.25)
        for r, n in enumerate(counts):
            if n:
                self.raw[cap - n:, r], self.val[cap - n:, r] = encode(rng.uniform(-amp, amp, size=(n, H)), split)
                self.words[cap - n:, r] = words(rng, n) if words else rng.randint(0, 50, size=n)


def cell_query(win, q_raw, g0, cnt, sent_len, idx, beam, N, frame=0, theta=THETA):
    """-> (rc, s [B * beam, ld_s], flags)"""
    B = len(idx)
    ld_s = min(win.cap, N) + 3
    s = torch.full((B * beam, ld_s), FILL, device=dev(), dtype=torch.float32)
    flags = torch.zeros(1, device=dev(), dtype=torch.int32)
    keep = [up(q_raw, np.float32), up(g0, np.int32), up(cnt, np.int32), up(sent_len, np.int32), up(win.raw, np.float32),
            up(win.count, np.int32), up(idx, np.int32)]
    torch.cuda.synchronize()
    rc = _lib.lib().jlm_cache_cell_query(keep[0].data_ptr(), win.H, int(win.split), H_SCALE, keep[1].data_ptr(), keep[2].data_ptr(),
                                         keep[3].data_ptr(), frame, B, beam, keep[4].data_ptr(), keep[5].data_ptr(), win.cap,
                                         len(win.count), keep[6].data_ptr(), N, theta, s.data_ptr(), ld_s, flags.data_ptr(), None)
    torch.cuda.synchronize()
    return rc, s.cpu().numpy(), int(flags.cpu()[0])


def row_query(win, q_rows, N, theta=THETA):
    """jlm_cache_query with query row r against cache row r -> s [n_src, ld_s]"""
    n_src = len(win.count)
    ld_s = min(win.cap, N) + 3
    s = torch.full((n_src, ld_s), FILL, device=dev(), dtype=torch.float32)
    flags = torch.zeros(1, device=dev(), dtype=torch.int32)
    keep = [up(win.raw, np.float32), up(q_rows, np.float32), up(win.cap - win.count, np.int32)]
    torch.cuda.synchronize()
    rc = _lib.lib().jlm_cache_query(keep[0].data_ptr(), win.cap, n_src, win.H, int(win.split), H_SCALE, keep[1].data_ptr(), n_src, None,
                                    win.cap, keep[2].data_ptr(), N, theta, s.data_ptr(), ld_s, flags.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0
    return s.cpu().numpy()


@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("H", [32, 64, 512])
def test_query_is_the_row_querys_bits(H, split):
    N = 70
    counts = [0, 1, 63, 64, 65, 70]
    win = Window(split, H, 70, counts, seed=H + split)
    rng = np.random.RandomState(7 * H + split)
    amp = min(0.999, 3.0 / H ** 0.25)
    worst = 0.0
    for beam in (1, 3, 17):
        # six cells, one per cache row (permuted), ragged counts: 0, below the beam, the beam; a sentence past its end; a row outside
        idx = np.array([4, 2, 5, 0, 1, 3, -1], dtype=np.int32)
        cnt = np.array([beam, max(beam - 1, 1), beam, beam, 0, 1, beam], dtype=np.int32)
        sent_len = np.array([3, 3, 3, 3, 3, 0, 3], dtype=np.int32)
        B = len(idx)
        q_raw, q_val = encode(rng.uniform(-amp, amp, size=(B * beam, H)), split)
        g0 = np.arange(B, dtype=np.int32) * beam
        rc, s, flags = cell_query(win, q_raw, g0, cnt, sent_len, idx, beam, N)
        assert rc == 0 and flags == 0
        want = np.full_like(s, FILL)
        for k in range(beam):                                              # slot k of every cell: one launch of the row kernel
            q_rows = np.zeros((len(counts), q_raw.shape[1]), dtype=np.float32)
            for j in range(B):
                if idx[j] >= 0:
                    q_rows[idx[j]] = q_raw[j * beam + k]
            ref = row_query(win, q_rows, N)
            for j in range(B):
                if idx[j] >= 0 and k < cnt[j] and sent_len[j] > 0:
                    want[j * beam + k] = ref[idx[j]]
        assert s.tobytes() == want.tobytes(), (H, split, beam)
        for j in range(B):
            r, n = idx[j], (counts[idx[j]] if idx[j] >= 0 else 0)
            for k in range(cnt[j] if sent_len[j] > 0 else 0):
                if n:
                    keys = win.val[win.cap - n:, r]
                    dot = keys @ q_val[j * beam + k]
                    bar = score_bar(split, H, THETA, float((np.abs(keys) @ np.abs(q_val[j * beam + k])).max()))
                    err = np.abs(s[j * beam + k, :n].astype(np.float64) - float(np.float32(THETA)) * dot).max()
                    worst = max(worst, err / bar)
                    assert err <= bar, (H, split, beam, j, k, err, bar)
        # a cell alone gives the bits it gives among the others
        j = 2
        rc, alone, _ = cell_query(win, q_raw[j * beam:(j + 1) * beam], g0[:1], cnt[j:j + 1], sent_len[j:j + 1], idx[j:j + 1], beam, N)
        assert rc == 0 and alone.tobytes() == s[j * beam:(j + 1) * beam].tobytes(), (H, split, beam)
    print("query H=%d split=%d: largest share of the score bar %.3f" % (H, split, worst))


def test_query_flags_a_product_that_is_not_finite():
    win = Window(0, 32, 4, [4], seed=1)
    q = np.full((1, 32), np.inf, dtype=np.float32)
    rc, s, flags = cell_query(win, q, [0], [1], [2], [0], 1, 4)
    assert rc == 0 and flags == 8 and not np.isfinite(s[0, :4]).any()


def test_refusals():
    win = Window(0, 32, 4, [4], seed=1)
    q = np.zeros((1, 32), dtype=np.float32)
    assert cell_query(win, q, [0], [1], [2], [0], 1, 4097)[0] == -1            # N > JLM_CACHE_MIX_MAX_N
    assert cell_query(win, q, [0], [1], [2], [0], 1, 0)[0] == -1
    assert cell_query(win, q, [0], [1], [2], [0], 1, 4, theta=-1.0)[0] == -1


# ------------------------------------------------------------------------------------------------------------------ the patch
def cell_patch(s, words, count, idx, N, lam, cnt, sent_len, beam, wl, wl_off, wl_out, edge, part=None, live_base=None, frame=0):
    """-> (rc, edge', s', lse [B * beam], flags)"""
    B = len(idx)
    cap, n_src = words.shape
    sd, ed = up(s, np.float32), up(edge, np.float32)
    lse = torch.full((B * beam,), -7.0, device=dev(), dtype=torch.float64)
    flags = torch.zeros(1, device=dev(), dtype=torch.int32)
    keep = [up(words, np.int32), up(count, np.int32), up(idx, np.int32), up(cnt, np.int32), up(sent_len, np.int32), up(wl, np.int32),
            up(wl_off, np.int32), up(wl_out, np.int32), up(np.arange(B), np.int32)]
    pd = up(part, np.float32) if part is not None else None
    lb = up(live_base, np.int32) if live_base is not None else None
    torch.cuda.synchronize()
    rc = _lib.lib().jlm_cache_cell_patch(sd.data_ptr(), s.shape[1], keep[0].data_ptr(), keep[1].data_ptr(), cap, n_src, keep[2].data_ptr(),
                                         N, lam, keep[3].data_ptr(), keep[4].data_ptr(), frame, B, beam, keep[5].data_ptr(),
                                         keep[6].data_ptr(), keep[8].data_ptr(), 0, keep[7].data_ptr(), ed.data_ptr(), pd.data_ptr() if pd is not None else None,
                                         B * beam, part.shape[0] if part is not None else 0, lb.data_ptr() if lb is not None else None,
                                         lse.data_ptr(), flags.data_ptr(), None)
    torch.cuda.synchronize()
    return rc, ed.cpu().numpy(), sd.cpu().numpy(), lse.cpu().numpy(), int(flags.cpu()[0])


def fold64(part, base, k):
    m = part[:, base + k, 0].astype(np.float64)
    sm = part[:, base + k, 1].astype(np.float64)
    top = m.max()
    return top + np.log((sm * np.exp(m - top)).sum())


@pytest.mark.parametrize("self_norm", [0, 1])
@pytest.mark.parametrize("N,J,n_parts", [(1, 1, 1), (17, 5, 7), (4096, 257, 40)])
def test_patch_against_the_definition(N, J, n_parts, self_norm):
    rng = np.random.RandomState(N + J + self_norm)
    beam, lam = 11, 0.3
    # cache rows: a full window, an empty one, one of one entry; sentence 3 has no cache row, sentence 4 is past its end
    count = np.array([N, 0, 1], dtype=np.int32)
    cap = N
    words = np.full((cap, 3), -1, dtype=np.int32)
    words[:, 0] = rng.randint(0, 6, size=N) if N > 1 else 3                # ids 0 .. 5: duplicates, id 0
    words[cap - 1:, 2] = 3
    if N >= 17:
        words[:, 0][rng.rand(N) < 0.5] = 9                                     # a word that takes half the window
    idx = np.array([0, 1, 2, 7, 0], dtype=np.int32)
    cnt = np.array([beam, beam, 3, beam, beam], dtype=np.int32)
    sent_len = np.array([2, 2, 2, 2, 0], dtype=np.int32)
    B = len(idx)
    # word lists: J positions a sentence, a word matching every entry of row 2's window (3), duplicates, id 0, words matching nothing
    lists = [np.concatenate(([3, 0, 9, 3, 400][:J], rng.randint(0, 12, size=max(J - 5, 0)))).astype(np.int32) for _ in range(B)]
    wl = np.concatenate(lists)
    wl_off = np.concatenate(([0], np.cumsum([len(x) for x in lists]))).astype(np.int32)
    wl_out = rng.permutation(len(wl)).astype(np.int32)                     # node ids: a permutation
    ld_s = N + 1
    s = np.full((B * beam, ld_s), NAN_BITS, dtype=np.float32)
    for j in range(B):
        n = count[idx[j]] if idx[j] < 3 else 0
        s[j * beam:j * beam + cnt[j], :n] = (4.0 * rng.standard_normal((cnt[j], n))).astype(np.float32)
    edge = (3.0 * rng.standard_normal(len(wl) * beam) - 6.0).astype(np.float32)
    part = live_base = None
    if not self_norm:
        part = np.stack([5.0 * rng.standard_normal((n_parts, B * beam)), rng.uniform(1.0, 50.0, size=(n_parts, B * beam))], axis=-1).astype(np.float32)
        live_base = np.array([0, 2 * beam, beam, 3 * beam, 4 * beam], dtype=np.int32)
    rc, e2, s2, lse, flags = cell_patch(s, words, count, idx, N, lam, cnt, sent_len, beam, wl, wl_off, wl_out, edge, part, live_base)
    assert rc == 0 and flags == 0
    lamf = float(np.float32(lam))
    log1m, log_rho = np.log1p(-lamf), np.log(lamf) - np.log1p(-lamf)
    want_same = edge.copy().reshape(len(wl), beam)
    got = e2.reshape(len(wl), beam)
    worst = 0.0
    for j in range(B):
        live = sent_len[j] > 0
        for k in range(beam):
            g = j * beam + k
            if live and k < cnt[j] and not self_norm:
                L = fold64(part, live_base[j], k)
                assert abs(lse[g] - L) <= 1e-6 * (1 + abs(L)), (j, k, lse[g], L)         # (f32 expf inside the fold)
            else:
                assert lse[g] == -7.0, (j, k)
        n = int(count[idx[j]]) if idx[j] < 3 else 0
        if not live or n == 0:
            continue                                                       # (its edge rows: checked bit for bit below)
        ww = words[cap - n:, idx[j]]
        for k in range(cnt[j]):
            sk = s[j * beam + k, :n].astype(np.float64)
            e = np.exp(sk - sk.max())
            L = 0.0 if self_norm else float(lse[j * beam + k])             # (the fold's own value: its error is not the patch's)
            for p in range(wl_off[j], wl_off[j + 1]):
                y = float(edge[wl_out[p] * beam + k])
                M = e[ww == wl[p]].sum()
                ref = L + log1m + np.logaddexp(y - L, log_rho + np.log(M) - np.log(e.sum())) if M > 0 else y + log1m
                bar = edge_bar(False, 0, N, 1.0, 0.0, ref, M > 0, spread=float(np.abs(sk - sk.max()).max()))
                err = abs(float(got[wl_out[p], k]) - ref)
                worst = max(worst, err / bar)
                assert err <= bar, (j, k, p, got[wl_out[p], k], ref, bar)
                want_same[wl_out[p], k] = got[wl_out[p], k]
    # everything else -- sentences without a window or past their end, slots past cnt -- keeps its bits
    assert got.tobytes() == want_same.tobytes()
    print("patch N=%d J=%d self_norm=%d: largest share of the edge bar %.3f" % (N, J, self_norm, worst))


@pytest.mark.parametrize("n_parts", [1, 7, 8, 9, 33, 40])
def test_patch_folds_the_bits_of_the_beam_steps_fused_fold(n_parts):
    """the lse rows the patch folds from a frame's slices = the rows jlm_beam_step's fused fold writes from the same part, live_base
    and cnt, bit for bit: 1 .. 40 slices, cells of 1, 5 and 20 rows (below and above the fold's 16 rows a pass), two frames"""
    from tests.test_gpu_beam_forms import State, cells, dyadic_inputs, lattice, _stream
    lib = _lib.lib()
    beam = 20
    P = lattice(beam, [cells([20, 3, 4], mix_last=False), cells([5, 3, 2], mix_last=False), cells([1, 2, 5], mix_last=False)])
    B, rmax, G = P["B"], P["rmax"], P["G"]
    rng = np.random.default_rng(n_parts)
    table = np.zeros((n_parts, G, 2), np.float32)
    table[:, :, 0] = rng.uniform(-5.0, 15.0, size=(n_parts, G)).astype(np.float32)
    table[:, :, 1] = np.exp(rng.uniform(0.0, np.log(1.0e4), size=(n_parts, G))).astype(np.float32)
    _lse0, edge = dyadic_inputs(P, 3)
    S = State(P, np.full(G, 1.0e30), edge, True)
    mine = torch.full((G,), -7.0, device=dev(), dtype=torch.float64)
    # a cache without a single entry: the patch folds and touches nothing else
    zeros = torch.zeros(8, device=dev(), dtype=torch.int32)
    idx = up(np.arange(B), np.int32)
    s = torch.zeros((rmax, 4), device=dev(), dtype=torch.float32)
    lists = torch.zeros(B + 1, device=dev(), dtype=torch.int32)
    part = torch.zeros((n_parts, rmax, 2), device=dev(), dtype=torch.float32)
    seen = []
    for f in range(P["F"]):
        if f >= 1:
            S.st.lse_part, S.st.ld_part, S.st.n_parts = part.data_ptr(), rmax, n_parts      # the fused step folds frame f - 1's rows
        assert lib.jlm_beam_step(S.lat, S.st, f, 0, P["max_cands"], _stream()) == 0
        S.sync()
        if f == P["F"] - 1:
            break
        nl = int(S.n_live[f].item())
        lv = S.live[f * rmax:f * rmax + nl].cpu().numpy().astype(np.int64)
        pn = np.zeros((n_parts, rmax, 2), np.float32)
        pn[:, :nl] = table[:, lv]
        part.copy_(up(pn, np.float32))
        edge_before = S.edge.clone()
        rc = lib.jlm_cache_cell_patch(s.data_ptr(), 4, zeros.data_ptr(), zeros.data_ptr(), 1, B, idx.data_ptr(), 4, 0.25,
                                      S.cnt.data_ptr() + 4 * f * B, S.ints["slen"].data_ptr(), f, B, beam, zeros.data_ptr(),
                                      lists.data_ptr(), idx.data_ptr(), 0, zeros.data_ptr(), S.edge.data_ptr(), part.data_ptr(), rmax,
                                      n_parts, S.live_base.data_ptr() + 4 * f * B, mine.data_ptr() + 8 * f * rmax, S.flags.data_ptr(),
                                      _stream())
        torch.cuda.synchronize()
        assert rc == 0 and torch.equal(S.edge, edge_before)
        seen.append(S.cnt[f * B:(f + 1) * B].cpu().numpy().tolist())
    got, cnt = S.lse.cpu().numpy(), S.cnt.cpu().numpy()
    assert seen[0] == [1, 1, 1] and seen[1] == [20, 5, 1], seen
    rows = 0
    for f in range(P["F"] - 1):
        for j in range(B):
            if f >= P["slen"][j]:
                continue
            g0, k = f * rmax + j * beam, int(cnt[f * B + j])
            assert mine[g0:g0 + k].cpu().numpy().tobytes() == got[g0:g0 + k].tobytes(), (n_parts, f, j)
            assert (mine[g0 + k:g0 + beam] == -7.0).all()
            rows += k
    assert rows >= 3 + 26 and int(S.flags.cpu()[0]) == 0


def test_patch_sanitises_a_log_normaliser_that_is_not_finite():
    beam, N = 3, 4
    words = np.array([[1], [2], [1], [3]], dtype=np.int32)
    s = np.zeros((beam, N), dtype=np.float32)
    edge = np.full(2 * beam, -5.0, dtype=np.float32)
    part = np.ones((2, beam, 2), dtype=np.float32)
    part[0, 1] = (0.0, np.inf)
    rc, e2, _s, lse, flags = cell_patch(s, words, [4], [0], N, 0.25, [beam], [2], beam, [1, 7], [0, 2], [0, 1], edge, part, [0])
    assert rc == 0 and flags == 1 and lse[1] == 1.0e30 and np.isfinite(lse).all() and np.isfinite(e2).all()
