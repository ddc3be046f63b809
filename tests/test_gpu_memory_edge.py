"""GPU: memory_gather_rows_kernel and memory_cell_patch_kernel as jlm_memory_gather_rows / jlm_memory_cell_patch launch them
(csrc/jlm_memory_edge.hip, include/jlm_hip.h), on scores, retrieved lists, word lists and slices the test writes
-- no model, no retrieval.

(a) The patch restates cache_cell_patch_kernel's arithmetic instead of sharing a header, so this file is what holds the two together:
    with every slot of a cell given the same list of words (and its own scores), ``edge`` and ``lse`` must be torch.equal to what
    jlm_cache_cell_patch writes from the same scores with that list as a full window (count = cap = K), over the same slices, cnt and
    live_base.
(b) Per-slot lists that differ -- repeated words, no match, a match in the last list position only -- against the float64 definition
    within decode_cache_budget.edge_bar at N_window = K (each case prints its measured share of the bar).
(c) n_q < K: entries j >= n_q are never read.  (d) The gather.  (e) A score that is not finite.  (f) Every refusal."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
from jlm_amd import _lib                                                                  # noqa: E402
from tests.decode_cache_budget import edge_bar                                            # noqa: E402
from tests.test_gpu_cache_edge import cell_patch as cache_patch, dev, fold64, up          # noqa: E402
from tests.test_gpu_cache_rows import NAN_BITS                                            # noqa: E402

pytestmark = pytest.mark.gpu

LAM = 0.3


def memory_patch(s, ret_words, N, K, lam, cnt, sent_len, beam, wl, wl_off, wl_out, edge, part, live_base, frame=0, n_rows=None, over=None):
    """-> (rc, edge', s', lse [B * beam], flags); ``over``: arguments replaced for a refusal"""
    B = len(cnt)
    n_rows = s.shape[0] if n_rows is None else n_rows
    sd, ed = up(s, np.float32), up(edge, np.float32)
    lse = torch.full((B * beam,), -7.0, device=dev(), dtype=torch.float64)
    flags = torch.zeros(1, device=dev(), dtype=torch.int32)
    keep = [up(ret_words, np.int32), up(cnt, np.int32), up(sent_len, np.int32), up(wl, np.int32), up(wl_off, np.int32), up(wl_out, np.int32),
            up(np.arange(B), np.int32), up(live_base, np.int32)]
    pd = up(part, np.float32) if part is not None else None
    a = dict(s=sd.data_ptr(), ld_s=s.shape[1], ret=keep[0].data_ptr(), n_rows=n_rows, N=N, K=K, lam=lam, cnt=keep[1].data_ptr(),
             slen=keep[2].data_ptr(), frame=frame, n_sent=B, beam=beam, wl=keep[3].data_ptr(), wl_off=keep[4].data_ptr(),
             wl_idx=keep[6].data_ptr(), wl_base=0, wl_out=keep[5].data_ptr(), edge=ed.data_ptr(), part=pd.data_ptr() if pd is not None else None,
             ld_part=n_rows, n_parts=part.shape[0] if part is not None else 0, base=keep[7].data_ptr(), lse=lse.data_ptr(),
             flags=flags.data_ptr(), stream=None)
    a.update(over or {})
    torch.cuda.synchronize()
    rc = _lib.lib().jlm_memory_cell_patch(*a.values())
    torch.cuda.synchronize()
    return rc, ed.cpu().numpy(), sd.cpu().numpy(), lse.cpu().numpy(), int(flags.cpu()[0])


def word_lists(rng, B, J, extra=()):
    lists = [np.concatenate((list(extra)[:J], rng.randint(0, 12, size=max(J - len(extra), 0)))).astype(np.int32) for _ in range(B)]
    wl = np.concatenate(lists)
    wl_off = np.concatenate(([0], np.cumsum([len(x) for x in lists]))).astype(np.int32)
    return wl, wl_off, rng.permutation(len(wl)).astype(np.int32)


# ------------------------------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("n_parts", [0, 1, 40])                             # 0: self-normalised (part = NULL)
@pytest.mark.parametrize("K", [1, 3, 64, 65, 1024])
def test_the_cache_patchs_bits(K, n_parts):
    rng = np.random.RandomState(K + n_parts)
    beam = 20
    cnt = np.array([1, 5, 17, 20, 20, 0], dtype=np.int32)                   # cells of 1, 5, 17 and 20 slots, a finished sentence, an empty cell
    sent_len = np.array([2, 2, 2, 2, 0, 2], dtype=np.int32)
    B = len(cnt)
    n_rows = B * beam
    live_base = (np.arange(B) * beam).astype(np.int32)                      # compact row = j * beam + k: both kernels read the same rows of s
    lists = rng.randint(0, 8, size=(K, B)).astype(np.int32)                 # one list a CELL: ids 0 .. 7, duplicates
    if K >= 64:
        lists[rng.rand(K, B) < 0.4] = 9                                     # a word that takes much of the list
    wl, wl_off, wl_out = word_lists(rng, B, 23, extra=(3, 0, 9, 3, 400))
    s = np.full((n_rows, K + 2), NAN_BITS, dtype=np.float32)
    for j in range(B):
        s[j * beam:j * beam + cnt[j], :K] = (4.0 * rng.standard_normal((cnt[j], K))).astype(np.float32)
    edge = (3.0 * rng.standard_normal(len(wl) * beam) - 6.0).astype(np.float32)
    part = None
    if n_parts:
        part = np.stack([5.0 * rng.standard_normal((n_parts, n_rows)), rng.uniform(1.0, 50.0, size=(n_parts, n_rows))], axis=-1).astype(np.float32)
    count, idx = np.full(B, K, dtype=np.int32), np.arange(B, dtype=np.int32)
    rc, want_e, _s, want_l, want_f = cache_patch(s, lists, count, idx, K, LAM, cnt, sent_len, beam, wl, wl_off, wl_out, edge, part,
                                                 live_base if n_parts else None)
    assert rc == 0 and want_f == 0
    ret_words = np.repeat(lists, beam, axis=1)                              # [K][n_rows]: every slot of cell j reads list j
    rc, got_e, got_s, got_l, got_f = memory_patch(s, ret_words, K, K, LAM, cnt, sent_len, beam, wl, wl_off, wl_out, edge, part, live_base)
    assert rc == 0 and got_f == 0
    assert torch.equal(torch.from_numpy(got_e), torch.from_numpy(want_e)) and (got_e != edge).any(), (K, n_parts)
    assert torch.equal(torch.from_numpy(got_l), torch.from_numpy(want_l)), (K, n_parts)
    assert got_s.tobytes() == s.tobytes()                                   # the scores are only read
    if n_parts:
        assert (got_l[:1] != -7.0).all() and (got_l[4 * beam:] == -7.0).all()


# ------------------------------------------------------------------------------------------------------------------ (b), (c)
def definition(s, ret_words, n_q, lam, cnt, sent_len, beam, wl, wl_off, wl_out, edge, L_of, live_base):
    """-> (ref, match) [positions, beam] float64 / bool: the float64 definition over the live slots, NaN elsewhere"""
    lamf = float(np.float32(lam))
    log1m, log_rho = np.log1p(-lamf), np.log(lamf) - np.log1p(-lamf)
    ref = np.full((len(wl), beam), np.nan)
    match = np.zeros((len(wl), beam), dtype=bool)
    spread = np.zeros((len(wl), beam))
    for j in range(len(cnt)):
        if sent_len[j] <= 0:
            continue
        for k in range(cnt[j]):
            c = live_base[j] + k
            sk = s[c, :n_q].astype(np.float64)
            e = np.exp(sk - sk.max())
            L = L_of(j, k)
            for p in range(wl_off[j], wl_off[j + 1]):
                y = float(edge[wl_out[p] * beam + k])
                hit = ret_words[:n_q, c] == wl[p]
                match[wl_out[p], k], spread[wl_out[p], k] = hit.any(), np.abs(sk - sk.max()).max()
                ref[wl_out[p], k] = L + log1m + np.logaddexp(y - L, log_rho + np.log(e[hit].sum()) - np.log(e.sum())) if hit.any() \
                    else y + log1m
    return ref, match, spread


@pytest.mark.parametrize("self_norm", [0, 1])
@pytest.mark.parametrize("N,K,J,n_parts", [(1, 1, 1, 1), (40, 17, 5, 7), (2000, 64, 70, 3), (5000, 1024, 257, 40), (5, 64, 9, 2)])
def test_per_slot_lists_against_the_definition(N, K, J, n_parts, self_norm):
    """every slot has its own list; (5, 64): n_q = 5 < K, the entries 5 .. 63 hold NaN scores and word ids that match, and are never read"""
    rng = np.random.RandomState(N + K + J + self_norm)
    beam, n_q = 11, min(K, N)
    cnt = np.array([beam, 3, beam, 1, beam], dtype=np.int32)
    sent_len = np.array([2, 2, 2, 2, 0], dtype=np.int32)
    B = len(cnt)
    n_rows = B * beam + 3
    live_base = np.array([0, 2 * beam, beam, 2 * beam + 3, 3 * beam + 3], dtype=np.int32)      # compact rows: packed, not j * beam
    wl, wl_off, wl_out = word_lists(rng, B, J, extra=(3, 0, 9, 3, 400))
    ret_words = rng.randint(0, 8, size=(K, n_rows)).astype(np.int32)        # ids 0 .. 7, repeated within a list; 400 and 8 .. 11 match nothing
    if n_q > 1:
        ret_words[:n_q - 1][ret_words[:n_q - 1] == 3] = 5                   # word 3: a match in the LAST list position only, in slot row 1
        ret_words[n_q - 1, 1] = 3
        ret_words[:n_q, 2] = 7                                              # row 2: one word takes the whole list
    else:
        ret_words[0, 0] = 3                                                 # a list of one entry: a match in row 0
    s = np.full((n_rows, K + 1), NAN_BITS, dtype=np.float32)
    s[:, :n_q] = (4.0 * rng.standard_normal((n_rows, n_q))).astype(np.float32)
    ret_words[n_q:] = 3                                                     # (c) beyond n_q: words that match, under NaN scores
    edge = (3.0 * rng.standard_normal(len(wl) * beam) - 6.0).astype(np.float32)
    part = None
    if not self_norm:
        part = np.stack([5.0 * rng.standard_normal((n_parts, n_rows)), rng.uniform(1.0, 50.0, size=(n_parts, n_rows))], axis=-1).astype(np.float32)
    rc, e2, s2, lse, flags = memory_patch(s, ret_words, N, K, LAM, cnt, sent_len, beam, wl, wl_off, wl_out, edge, part, live_base)
    assert rc == 0 and flags == 0 and s2.tobytes() == s.tobytes()
    got = e2.reshape(len(wl), beam)
    for j in range(B):
        for k in range(beam):
            if sent_len[j] > 0 and k < cnt[j] and not self_norm:
                L = fold64(part, live_base[j], k)
                assert abs(lse[j * beam + k] - L) <= 1e-6 * (1 + abs(L)), (j, k)          # (f32 expf inside the fold)
            else:
                assert lse[j * beam + k] == -7.0, (j, k)
    ref, match, spread = definition(s, ret_words, n_q, LAM, cnt, sent_len, beam, wl, wl_off, wl_out, edge,
                                    (lambda j, k: 0.0) if self_norm else (lambda j, k: float(lse[j * beam + k])), live_base)
    live = ~np.isnan(ref)
    assert live.sum() == sum(int(cnt[j]) * (wl_off[j + 1] - wl_off[j]) for j in range(B) if sent_len[j] > 0)
    assert match[live].any() and not match[live].all()
    worst = 0.0
    for p, k in zip(*np.nonzero(live)):
        bar = edge_bar(False, 0, K, 1.0, 0.0, ref[p, k], match[p, k], spread=float(spread[p, k]))
        err = abs(float(got[p, k]) - ref[p, k])
        worst = max(worst, err / bar)
        assert err <= bar, (p, k, got[p, k], ref[p, k], bar)
    # everything else -- a finished sentence, slots past cnt -- keeps its bits
    assert got[~live].tobytes() == edge.reshape(len(wl), beam)[~live].tobytes()
    print("patch N=%d K=%d J=%d self_norm=%d: largest share of the edge bar %.3f" % (N, K, J, self_norm, worst))


# ------------------------------------------------------------------------------------------------------------------ (e)
def test_a_score_that_is_not_finite_keeps_the_slots_logits():
    rng = np.random.RandomState(5)
    beam, K = 5, 16
    cnt, sent_len, live_base = np.array([5, 5], dtype=np.int32), np.array([3, 3], dtype=np.int32), np.array([0, 5], dtype=np.int32)
    wl, wl_off, wl_out = word_lists(rng, 2, 6)
    ret_words = rng.randint(0, 12, size=(K, 10)).astype(np.int32)
    s = rng.standard_normal((10, K)).astype(np.float32)
    edge = (rng.standard_normal(len(wl) * beam) - 3.0).astype(np.float32)
    rc, clean, _s, _l, flags = memory_patch(s, ret_words, 100, K, LAM, cnt, sent_len, beam, wl, wl_off, wl_out, edge, None, live_base)
    assert rc == 0 and flags == 0
    for bad, c in ((np.inf, 2), (-np.inf, 7), (np.nan, 9)):
        s2 = s.copy()
        s2[c, K - 1] = bad
        rc, got, _s, _l, flags = memory_patch(s2, ret_words, 100, K, LAM, cnt, sent_len, beam, wl, wl_off, wl_out, edge, None, live_base)
        assert rc == 0 and flags == 8
        want = clean.reshape(len(wl), beam).copy()
        j, k = divmod(c, beam)
        rows = wl_out[wl_off[j]:wl_off[j + 1]]
        want[rows, k] = edge.reshape(len(wl), beam)[rows, k]               # the slot keeps its logits; every other slot is patched
        assert got.reshape(len(wl), beam).tobytes() == want.tobytes(), (bad, c)


# ------------------------------------------------------------------------------------------------------------------ (d)
@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("H", [32, 512])
def test_gather_copies_the_live_rows_and_nothing_else(H, split):
    """live counts 0, 1, 33 and rmax; rows beyond the live count keep a poison pattern; both state-row formats (a row is 4 H bytes: f32
    values, or the f16 pairs of split rows -- any bit pattern, NaN patterns among them)"""
    rng = np.random.RandomState(H + split)
    rmax, pool_rows = 40, 200
    if split:
        pool = rng.randint(-2 ** 31, 2 ** 31, size=(pool_rows, H), dtype=np.int64).astype(np.int32)
    else:
        pool = rng.standard_normal((pool_rows, H)).astype(np.float32).view(np.int32)
    pd = torch.from_numpy(pool).to(dev())
    rows = rng.permutation(pool_rows)[:rmax].astype(np.int32)
    rd = up(rows, np.int32)
    lib = _lib.lib()
    for n_live in (0, 1, 33, rmax):
        for counted in (True, False):                                      # the live count from the device, or n_rows_max alone
            out = torch.full((rmax, H), 0x7FC0DEAD, device=dev(), dtype=torch.int32)
            nd = up([n_live if counted else 10 ** 6], np.int32)
            torch.cuda.synchronize()
            rc = lib.jlm_memory_gather_rows(pd.data_ptr(), H, pool_rows, rd.data_ptr(), nd.data_ptr() if counted else None,
                                            rmax if counted else n_live, out.data_ptr(), None)
            torch.cuda.synchronize()
            assert rc == 0
            got = out.cpu().numpy()
            assert np.array_equal(got[:n_live], pool[rows[:n_live]]) and (got[n_live:] == 0x7FC0DEAD).all(), (H, split, n_live, counted)
    # a row index outside the pool copies nothing
    out = torch.full((rmax, H), 0x7FC0DEAD, device=dev(), dtype=torch.int32)
    wild = up([3, -1, pool_rows, 5], np.int32)
    assert lib.jlm_memory_gather_rows(pd.data_ptr(), H, pool_rows, wild.data_ptr(), None, 4, out.data_ptr(), None) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got[[0, 3]], pool[[3, 5]]) and (got[[1, 2]] == 0x7FC0DEAD).all() and (got[4:] == 0x7FC0DEAD).all()


# ------------------------------------------------------------------------------------------------------------------ (f)
def test_refusals():
    rng = np.random.RandomState(1)
    beam, K = 3, 8
    cnt, sent_len, live_base = np.array([3], dtype=np.int32), np.array([2], dtype=np.int32), np.array([0], dtype=np.int32)
    wl, wl_off, wl_out = word_lists(rng, 1, 4)
    ret_words = rng.randint(0, 12, size=(K, 3)).astype(np.int32)
    s = rng.standard_normal((3, K)).astype(np.float32)
    edge = rng.standard_normal(len(wl) * beam).astype(np.float32)
    part = np.ones((2, 3, 2), dtype=np.float32)
    call = lambda **bad: memory_patch(s, ret_words, 20, K, bad.pop("lam_", LAM), cnt, sent_len, beam, wl, wl_off, wl_out, edge, part, live_base,
                                      over=bad)
    rc, clean, _s, _l, _f = call()
    assert rc == 0 and (clean != edge).any()
    for bad in (dict(lam_=0.0), dict(lam_=1.0), dict(lam_=float("nan")), dict(K=0), dict(K=1025), dict(ld_s=K - 1), dict(n_rows=0),
                dict(n_rows=65536), dict(N=0), dict(beam=0), dict(beam=1025), dict(n_sent=65536), dict(n_sent=-1), dict(frame=-1),
                dict(s=None), dict(ret=None), dict(cnt=None), dict(slen=None), dict(wl=None), dict(wl_off=None), dict(wl_idx=None),
                dict(wl_out=None), dict(edge=None), dict(base=None), dict(wl_base=-1), dict(lse=None), dict(n_parts=0), dict(ld_part=0)):
        rc, got, _s, lse, flags = call(**bad)
        assert rc == -1 and got.tobytes() == edge.tobytes() and (lse == -7.0).all() and flags == 0, bad
    # a misaligned pointer
    sd = up(s, np.float32)
    rc, got, _s, _l, _f = call(s=sd.data_ptr() + 2)
    assert rc == -1 and got.tobytes() == edge.tobytes()
    # nothing to do is no refusal
    assert call(n_sent=0)[0] == 0
    # the gather
    lib = _lib.lib()
    pool = torch.zeros((8, 32), device=dev())
    out = torch.full((4, 32), 9.0, device=dev())
    rows = up([1, 2, 3, 4], np.int32)
    ok = dict(h=pool.data_ptr(), H=32, pool=8, rows=rows.data_ptr(), ndev=None, n=4, out=out.data_ptr(), stream=None)
    for bad in (dict(H=0), dict(H=30), dict(n=-1), dict(n=65536), dict(h=None), dict(rows=None), dict(out=None), dict(pool=0), dict(pool=-1),
                dict(h=pool.data_ptr() + 4), dict(out=out.data_ptr() + 8)):
        assert lib.jlm_memory_gather_rows(*dict(ok, **bad).values()) == -1, bad
    torch.cuda.synchronize()
    assert bool((out == 9.0).all())
    assert lib.jlm_memory_gather_rows(*dict(ok, n=0).values()) == 0
