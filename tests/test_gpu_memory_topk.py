"""GPU: memory_topk_score_kernel / memory_topk_select_kernel as jlm_memory_topk launches them (csrc/jlm_memory_topk.hip,
include/jlm_hip.h), on keys and query rows the test writes -- no model.  The reference is the float64 product of the DECODED operands
(split rows: (hi + lo) / h_scale); the bar of a score is derived in tests/memory_topk_budget.py, not measured.

Per live row, with idx / s / words the returned lists and s64_i = theta (h_q . k_i) in float64:
  (a) the indices are distinct and in [0, N), words[j] = key_words[idx[j]], s is non-increasing and idx ascends inside a run of equal
      score bits;
  (b) |s_j - s64[idx_j]| <= bar of the pair;
  (c) every index NOT returned has s64 <= min_j s64[idx_j] + 2 bar (bar: the row's largest) -- exact, no case left out;
  (d) with key rows duplicated exactly across tile, workgroup-range and chunk borders the lower indices win, bit for bit;
  (e) a row's bits do not depend on its position, its companions, the live count, the workspace's size, or what outputs and workspace
      held before;
  (f) rows that are not live and entries >= n_q keep what they held;
  (g) the flag goes up for an inf key, and the refusals fire.
Every shape runs with the workspace that holds the whole memory in one chunk, with the least jlm_memory_topk_workspace_bytes allows (a
chunk of 32 keys: as many chunks as N has tiles, the last one ragged) and, where N has more than 512 keys, with a chunk of 512.
Largest share of the bar seen: DESIGN.md section 29.
"""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
from jlm_amd import _lib                                                                  # noqa: E402
from tests import poison                                                                  # noqa: E402
from tests.memory_topk_budget import score_bar                                            # noqa: E402
from tests.test_gpu_cache_rows import H_SCALE, NAN_BITS, encode                            # noqa: E402

pytestmark = pytest.mark.gpu

FILL = 123.0                                                                               # what s holds before a launch
IFILL = -7                                                                                 # ... and ret_words / ret_idx
WORST = [0.0]


class Case:
    """keys [N, H] / key_words [N] and R query rows [R, H]"""

    def __init__(self, split, H, N, R, seed, n_words=11):
        rng = np.random.RandomState(seed)
        amp = min(0.999, 3.0 / H ** 0.25)                                  # h . k of a few units either way at every H
        self.split, self.H, self.N, self.R = split, H, N, R
        self.k_raw, self.k_val = encode(rng.uniform(-amp, amp, size=(N, H)), split)
        self.q_raw, self.q_val = encode(rng.uniform(-amp, amp, size=(R, H)), split)
        self.k_words = rng.randint(0, n_words, size=N).astype(np.int32)


def full_bytes(N, R, K):
    return R * ((N + 31) // 32 * 32 * 4 + K * 8)


def launch(cs, theta, K, ws_bytes=None, extra=0, n_dev=None, fill=None, flags=True, **over):
    """the launcher over cs's rows with ``extra`` rows more in every buffer (NaN query rows, never live: *n_dev = cs.R unless given);
    ``fill``: a poison.Fill for the workspace and the outputs' prefill.  -> (rc, s [R + extra, K + 3], words, idx [K, R + extra + 1],
    flags)"""
    dev = torch.device("cuda", torch.cuda.current_device())
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    Rm, n_rows, ld_s = cs.R + extra, cs.R + extra + 1, K + 3
    q_raw = np.concatenate([cs.q_raw, np.full((extra, cs.q_raw.shape[1]), NAN_BITS, dtype=np.float32)]) if extra else cs.q_raw
    keys, kw, qr = up(cs.k_raw, np.float32), up(cs.k_words, np.int32), up(q_raw, np.float32)
    nd = up(np.array([cs.R if n_dev is None else n_dev]), np.int32)
    lib = _lib.lib()
    need = int(lib.jlm_memory_topk_workspace_bytes(cs.N, Rm, K))
    ws_bytes = full_bytes(cs.N, Rm, K) if ws_bytes is None else ws_bytes
    ws = torch.zeros(max(ws_bytes // 4, 4), device=dev, dtype=torch.float32)
    s = torch.full((Rm, ld_s), FILL, device=dev, dtype=torch.float32)
    words = torch.full((K, n_rows), IFILL, device=dev, dtype=torch.int32)
    idx = torch.full((K, n_rows), IFILL, device=dev, dtype=torch.int32)
    if fill is not None:
        for t in (ws, s):
            poison.fill_tensor(t, fill)
        for t in (words, idx):
            t.fill_(-1 if fill.byte == 0xFF else 1)
    fl = torch.zeros(1, device=dev, dtype=torch.int32)
    a = dict(keys=keys.data_ptr(), key_words=kw.data_ptr(), N=cs.N, H=cs.H, split=int(cs.split), h_scale=H_SCALE, q_rows=qr.data_ptr(),
             n_rows_max=Rm, n_dev=nd.data_ptr(), theta=float(theta), K=K, s=s.data_ptr(), ld_s=ld_s, ret_words=words.data_ptr(),
             ret_idx=idx.data_ptr(), n_rows=n_rows, workspace=ws.data_ptr(), workspace_bytes=ws_bytes, flags=fl.data_ptr() if flags else None,
             stream=None)
    for k, v in over.items():                                                  # (as_theta / as_K: the argument alone, the buffers as made)
        a[k[3:] if k.startswith("as_") else k] = v
    torch.cuda.synchronize()
    rc = lib.jlm_memory_topk(*a.values())
    torch.cuda.synchronize()
    assert need <= full_bytes(cs.N, Rm, K)
    return rc, s.cpu().numpy(), words.cpu().numpy(), idx.cpu().numpy(), int(fl.cpu()[0])


def check(cs, theta, K, tag, live=None, **kw):
    """(a), (b), (c) and (f) of one launch -> (s, words, idx)"""
    rc, s, words, idx, flags = launch(cs, theta, K, **kw)
    assert rc == 0 and flags == 0, (tag, rc, flags)
    live = cs.R if live is None else live
    n_q = min(K, cs.N)
    th = float(np.float32(theta))
    # (f)
    assert np.all(s[live:] == np.float32(FILL)) and np.all(s[:, n_q:] == np.float32(FILL)), tag
    for out in (words, idx):
        assert np.all(out[:, live:] == IFILL) and np.all(out[n_q:] == IFILL), tag
    worst = 0.0
    for r in range(live):
        i_r, s_r = idx[:n_q, r].astype(np.int64), s[r, :n_q]
        # (a)
        assert i_r.min() >= 0 and i_r.max() < cs.N and len(set(i_r.tolist())) == n_q, (tag, r)
        assert np.array_equal(words[:n_q, r], cs.k_words[i_r]), (tag, r)
        assert np.all(s_r[1:] <= s_r[:-1]), (tag, r)
        same = s_r[1:].view(np.uint32) == s_r[:-1].view(np.uint32)
        assert np.all(i_r[1:][same] > i_r[:-1][same]), (tag, r)
        # (b)
        s64 = th * (cs.k_val @ cs.q_val[r])
        bar = score_bar(cs.split, cs.H, theta, np.abs(cs.k_val) @ np.abs(cs.q_val[r]))
        err = np.abs(s_r.astype(np.float64) - s64[i_r])
        assert np.all(err <= bar[i_r]), (tag, r, float(err.max()))
        if th > 0:
            worst = max(worst, float((err / bar[i_r]).max()))
        # (c)
        rest = np.ones(cs.N, dtype=bool)
        rest[i_r] = False
        if rest.any():
            assert s64[rest].max() <= s64[i_r].min() + 2 * bar.max(), (tag, r)
    WORST[0] = max(WORST[0], worst)
    print("%s: %d rows, n_q %d, max err / bar %.3f (largest share so far %.3f)" % (tag, live, n_q, worst, WORST[0]))
    return s, words, idx


def workspaces(N, Rm, K):
    """the workspace sizes a shape runs with, and the chunks each gives"""
    lib = _lib.lib()
    out = [full_bytes(N, Rm, K), int(lib.jlm_memory_topk_workspace_bytes(N, Rm, K))]
    if N > 512:
        out.append(Rm * (512 * 4 + K * 8))
    chunks = [int(lib.jlm_memory_topk_chunk_keys(N, Rm, K, b)) for b in out]
    assert chunks[0] == (N + 31) // 32 * 32 and chunks[1] == 32 and chunks[2:] in ([], [512])
    return out


# Both row formats x every N -- {1, 31, 33, 64}: the edges of a tile and of a tile pair; {511, 513, 1057}: one workgroup's range of 512
# keys less a key, a second range of one key, three ranges with a ragged last one -- with H and the rows cycling through their values
# and two K per shape, so that each value meets both formats, K < N and K >= N, and K on both sides of the select's 256 threads.
NS = [1, 31, 33, 64, 511, 513, 1057]
HS = [32, 96, 512]
ROWS = [1, 3, 33, 65]
KS = [1, 7, 64, 65, 1024]
SHAPES = [(split, HS[(i + split) % 3], N, ROWS[(i + 2 * split) % 4], KS[(i + j + split) % 5])
          for split in (0, 1) for i, N in enumerate(NS) for j in (0, 2)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%s-H%d-N%d-R%d-K%d" % (("f32", "split")[s[0]], s[1], s[2], s[3], s[4]))
def test_shapes(shape):
    split, H, N, R, K = shape
    cs = Case(split, H, N, R, seed=N + 7 * H + R + K)
    base = None
    for b in workspaces(N, R + 2, K):
        got = check(cs, 0.7, K, "shape %s ws %d" % (shape, b), ws_bytes=b, extra=2)
        if base is None:
            base = got
        for x, y, what in zip(got, base, ("s", "words", "idx")):                          # (e): the workspace's size
            assert poison.bits(x) == poison.bits(y), (shape, b, poison.first_difference(x, y, what))


@pytest.mark.parametrize("split", [0, 1])
def test_duplicated_keys_resolve_to_the_lower_index(split):
    """(d): N = 1057 key rows that repeat 40 distinct ones (i and i + 40 hold the same bits): a group's members share their score's
    bits, so a group's returned members are its lowest indices, adjacent and ascending, at every K and chunk; theta = 0 makes every
    entry tie: exactly the indices 0 .. n_q - 1 in order, with the score +0"""
    H, N, R, G = 96, 1057, 3, 40
    cs = Case(split, H, N, R, seed=77 + split)
    cs.k_raw, cs.k_val = cs.k_raw[np.arange(N) % G].copy(), cs.k_val[np.arange(N) % G].copy()
    for K in (7, 100, 1024):
        base = None
        for b in workspaces(N, R, K):
            s, words, idx = check(cs, 1.3, K, "duplicates K %d ws %d" % (K, b), ws_bytes=b)
            n_q = min(K, N)
            for r in range(R):
                i_r, s_r = idx[:n_q, r], s[r, :n_q]
                for g in range(G):
                    at = np.flatnonzero(i_r % G == g)
                    if len(at):
                        assert np.array_equal(i_r[at], g + G * np.arange(len(at))), (K, b, r, g)
                        assert np.array_equal(at, at[0] + np.arange(len(at))), (K, b, r, g)
                        assert len(set(s_r[at].view(np.uint32).tolist())) == 1, (K, b, r, g)
            if base is None:
                base = (s, words, idx)
            assert poison.bits((s, words, idx)) == poison.bits(base), (K, b)
            rc, s0, _w0, idx0, fl = launch(cs, 0.0, K, ws_bytes=b)
            assert rc == 0 and fl == 0
            assert np.array_equal(idx0[:n_q, :R], np.repeat(np.arange(n_q)[:, None], R, axis=1))
            assert np.all(s0[:R, :n_q].view(np.uint32) == 0)


@pytest.mark.parametrize("split", [0, 1])
def test_a_rows_bits_do_not_depend_on_the_launch(split):
    """(e): one row launched alone, among 65 rows (another column, another block), with most rows not live, at every workspace size
    and over both prefills of outputs and workspace: the same bits"""
    H, N, K = 64, 1057, 65
    big = Case(split, H, N, 65, seed=33)
    s, words, idx = check(big, 0.7, K, "65 rows")
    part = check(big, 0.7, K, "65 rows, 34 live", live=34, n_dev=34)
    assert poison.bits([x[..., :34] if x is not part[0] else x[:34] for x in part]) == poison.bits([s[:34], words[:, :34], idx[:, :34]])
    for r in (0, 31, 32, 64):
        one = Case(split, H, N, 1, seed=33)
        one.k_raw, one.k_val, one.k_words = big.k_raw, big.k_val, big.k_words
        one.q_raw, one.q_val = big.q_raw[r:r + 1].copy(), big.q_val[r:r + 1]
        for b, fill in zip(workspaces(N, 1, K), (None,) + poison.FILLS):
            rc, s1, w1, i1, fl = launch(one, 0.7, K, ws_bytes=b, fill=fill)
            assert rc == 0 and fl == 0
            assert poison.bits((s1[0, :K], w1[:, 0], i1[:, 0])) == poison.bits((s[r, :K], words[:, r], idx[:, r])), (r, b, fill)


@pytest.mark.parametrize("split", [0, 1])
def test_flag(split):
    """an inf planted in a key sets flag bit 0; an unflagged launch leaves the flag at 0; a NULL flag pointer is accepted"""
    cs = Case(split, 64, 513, 3, seed=41)
    assert launch(cs, 0.5, 7)[4] == 0
    if split:
        cs.k_raw[512].view(np.uint16)[3] = 0x7c00                               # f16 +inf in a hi half of the last key
    else:
        cs.k_raw[512, 5] = np.inf
    rc, _s, _w, _i, fl = launch(cs, 0.5, 7)
    assert rc == 0 and fl == 1
    rc, _s, _w, _i, fl = launch(cs, 0.5, 7, flags=False)
    assert rc == 0 and fl == 0


def test_refusals_on_the_device_library():
    """the launcher's -1 cases launch nothing (the outputs keep their prefill), an empty launch returns 0"""
    cs = Case(1, 64, 40, 2, seed=3)
    K = 7
    lib = _lib.lib()
    need = int(lib.jlm_memory_topk_workspace_bytes(cs.N, cs.R, K))
    assert need == cs.R * (32 * 4 + K * 8)
    for args in ((0, 2, 7), (1 << 24 | 1, 2, 7), (40, -1, 7), (40, 2, 0), (40, 2, 1025)):
        assert lib.jlm_memory_topk_workspace_bytes(*args) == 0 and lib.jlm_memory_topk_chunk_keys(*args, 1 << 20) == 0
    assert lib.jlm_memory_topk_chunk_keys(cs.N, cs.R, K, need - 1) == 0 and lib.jlm_memory_topk_chunk_keys(cs.N, cs.R, K, need) == 32
    probe = launch(cs, 0.5, K)
    assert probe[0] == 0 and not np.any(probe[1][:, :K] == np.float32(FILL))

    def refused(**kw):
        rc, s, words, idx, fl = launch(cs, 0.5, K, **kw)
        assert np.all(s == np.float32(FILL)) and np.all(words == IFILL) and np.all(idx == IFILL) and fl == 0, kw
        return rc

    for kw in (dict(N=0), dict(N=-5), dict(N=(1 << 24) + 1), dict(H=0), dict(H=48), dict(keys=None), dict(key_words=None), dict(q_rows=None),
               dict(s=None), dict(ret_words=None), dict(workspace=None), dict(as_theta=-1.0), dict(as_theta=float("inf")),
               dict(as_theta=float("nan")), dict(h_scale=0.0), dict(h_scale=-2.0), dict(as_K=0), dict(as_K=1025), dict(ld_s=K - 1), dict(n_rows_max=-1), dict(n_rows_max=4),
               dict(n_rows=65536), dict(ws_bytes=need - 4), dict(workspace_bytes=0)):
        assert refused(**kw) == -1, kw
    dev = torch.device("cuda", torch.cuda.current_device())
    odd = torch.zeros(cs.N * cs.H + 4096, device=dev, dtype=torch.float32)
    for kw in (dict(keys=odd.data_ptr() + 4), dict(q_rows=odd.data_ptr() + 8), dict(workspace=odd.data_ptr() + 8), dict(key_words=odd.data_ptr() + 2),
               dict(s=odd.data_ptr() + 1), dict(ret_words=odd.data_ptr() + 2), dict(ret_idx=odd.data_ptr() + 2), dict(as_n_dev=odd.data_ptr() + 2)):
        assert refused(**kw) == -1, kw
    assert refused(n_rows_max=0) == 0
    rc, s, words, idx, fl = launch(cs, 0.5, K, ret_idx=None)                      # ret_idx may be NULL
    assert rc == 0 and fl == 0 and np.all(idx == IFILL) and poison.bits((s, words)) == poison.bits(probe[1:3])
