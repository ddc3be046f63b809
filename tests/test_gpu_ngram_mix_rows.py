"""GPU: ngram_mix_rows_kernel and ngram_hist_advance_kernel as jlm_ngram_mix_rows / jlm_ngram_hist_advance launch them
(csrc/jlm_ngram_mix.hip, include/jlm_hip.h), on tables, histories and logits the test writes -- no model.  Every patched logit is
checked against ``jlm_amd.ngram.mixed_logits`` (float64 over the f32 table values) within the bar of tests/ngram_mix_budget.py, whose
docstring holds the derivation term by term; nothing there is measured, and each test prints its measured maximum as a share of the
bar.  Exact values are asserted where the definition gives them: a word with q = -inf keeps its bits, rows that are not live and
everything beyond V keep every byte, a row gives the same bits alone as inside a batch, and two launches give the same bits."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
from jlm_amd import _lib                                                                  # noqa: E402
from jlm_amd.ngram import NGramTable, mixed_logits, pack, successor_tensors               # noqa: E402
from tests.ngram_mix_budget import y_bar                                                  # noqa: E402
from tests.row_lse_pin import CASES as LSE_CASES, LAM as LSE_LAM, expected_bits, pin_row  # noqa: E402

pytestmark = pytest.mark.gpu

NAN_BITS = np.frombuffer(np.uint32(0x7fc12345).tobytes(), dtype=np.float32)[0]           # the poison beyond V and beyond the live rows
GOLDEN = 0x9E3779B97F4A7C15


def make_table(V, seed, n_bi, n_tri, full_ctx=None):
    """A rounded order-3 table over V words with the cases the walk has to tell apart: word 1 has no unigram (q = -inf wherever no
    longer n-gram names it) when V > 3; bigrams and trigrams drawn at random, half of the bigrams with a back-off weight -- so there
    are contexts with a weight and no successors and contexts with successors and no weight --, some unigrams without a weight;
    ``full_ctx`` = (u, v): that context is followed by EVERY word (a list that covers the vocabulary)."""
    rng = np.random.RandomState(seed)
    ent = {}
    for w in range(V):
        if not (w == 1 and V > 3):
            ent[(w,)] = (-rng.uniform(0.1, 12.0), rng.uniform(-2.0, 1.0) if w % 3 else 0.0)
    for _ in range(n_bi):
        v, w = int(rng.randint(V)), int(rng.randint(V))
        ent[(v, w)] = (-rng.uniform(0.1, 9.0), rng.uniform(-2.0, 1.0) if rng.rand() < 0.5 else 0.0)
    for _ in range(n_tri):
        u, v, w = int(rng.randint(V)), int(rng.randint(V)), int(rng.randint(V))
        ent[(u, v, w)] = (-rng.uniform(0.1, 6.0), 0.0)
    if full_ctx is not None:
        for w in range(V):
            ent[tuple(full_ctx) + (w,)] = (-rng.uniform(0.1, 6.0), 0.0)
    ks = sorted(ent, key=pack)
    return NGramTable([pack(k) for k in ks], [ent[k][0] for k in ks], [ent[k][1] for k in ks], 3).rounded()


def histories(table, V, arr):
    """the (u, v) of the issue's list that this table has, each named"""
    n1, n2 = np.searchsorted(table.keys, [1 << 21, 1 << 42])
    bi = {((k >> 21) - 1, (k & 0x1FFFFF) - 1): b for k, b in zip(table.keys[n1:n2].tolist(), table.bow[n1:n2].tolist())}
    tri_ctx = {((k >> 42) - 1, ((k >> 21) & 0x1FFFFF) - 1) for k in table.keys[n2:].tolist()}
    uni_bow = {(k - 1): b for k, b in zip(table.keys[:n1].tolist(), table.bow[:n1].tolist())}
    has_bi = {v for v, _ in bi}
    out = {"none": (-1, -1)}
    pick = lambda name, it: out.setdefault(name, next(iter(it), None))
    pick("bigram only, bow(v) != 0", ((-1, v) for v in range(V) if uni_bow.get(v, 0.0) != 0.0 and v in has_bi))
    pick("bigram only, bow(v) = 0", ((-1, v) for v in range(V) if uni_bow.get(v, 0.0) == 0.0 and v in has_bi))
    pick("no successor of v at all", ((-1, v) for v in range(V) if v not in has_bi))
    pick("trigram context with bow(u v)", (c for c in sorted(tri_ctx) if bi.get(c, 0.0) != 0.0))
    pick("trigram context without bow(u v)", (c for c in sorted(tri_ctx) if bi.get(c, 0.0) == 0.0))
    pick("bow(u v) and no trigram successor", (c for c in sorted(bi) if bi[c] != 0.0 and c not in tri_ctx))
    pick("no context (u, v)", ((u, v) for u in range(V) for v in range(V) if (u, v) not in tri_ctx and bi.get((u, v), 0.0) == 0.0))
    pick("v without a unigram", ((0, 1) for _ in range(1) if V > 3))
    # the context that sits at displacement max_probe in the map
    cap, keys = 1 << arr["log2cap"], arr["ctx_keys"]
    for s in np.flatnonzero(keys):
        k = int(keys[s])
        home = ((k * GOLDEN) & ((1 << 64) - 1)) >> (64 - arr["log2cap"])
        if (int(s) - home) % cap == arr["max_probe"]:
            out["displacement max_probe = %d" % arr["max_probe"]] = ((k >> 21) - 1, (k & 0x1FFFFF) - 1)
            break
    return {k: v for k, v in out.items() if v is not None}


def rows_struct(tens, arr, **over):
    t = _lib.NgramRows()
    for name in ("uni_lp", "uni_bow", "bi_off", "bi_w", "bi_lp", "tri_off", "tri_w", "tri_lp", "tri_bow", "ctx_keys", "ctx_vals"):
        setattr(t, name, tens[name].data_ptr())
    t.n_bi, t.n_tri, t.n_ctx = int(arr["bi_w"].size), int(arr["tri_w"].size), int(arr["n_ctx"])
    t.log2cap, t.max_probe = int(arr["log2cap"]), int(arr["max_probe"])
    for k, v in over.items():
        setattr(t, k, v)
    return t


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def launch(table, V, y, hist, lam, order, self_norm=0, live=None, n_dev=None, struct_over=None):
    """-> (rc, y' [R, ld], flags)"""
    tens, arr = successor_tensors(table, V, dev())
    t = rows_struct(tens, arr, **(struct_over or {}))
    yd = torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32)).to(dev())
    hd = torch.from_numpy(np.ascontiguousarray(hist, dtype=np.int32)).to(dev())
    flags = torch.zeros(1, device=dev(), dtype=torch.int32)
    nd = torch.tensor([n_dev], device=dev(), dtype=torch.int32) if n_dev is not None else None
    torch.cuda.synchronize()
    rc = _lib.lib().jlm_ngram_mix_rows(yd.data_ptr(), y.shape[1], V, self_norm, ctypes.byref(t), hd.data_ptr(),
                                       y.shape[0] if live is None else live, nd.data_ptr() if nd is not None else None, lam, order,
                                       flags.data_ptr(), None)
    torch.cuda.synchronize()
    return rc, yd.cpu().numpy(), int(flags.cpu()[0])


def make_rows(V, R, seed):
    rng = np.random.RandomState(seed)
    ld = (V + 3) // 4 * 4 + 4
    y = np.full((R, ld), NAN_BITS, dtype=np.float32)
    y[:, :V] = (3.0 * rng.standard_normal((R, V))).astype(np.float32)
    return y


def same_bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def context_in_use(hist, order):
    u, v = int(hist[0]), int(hist[1])
    if order < 2 or v < 0:
        return []
    return [v] if order < 3 or u < 0 else [u, v]


def check_rows(table, V, y, hist, y2, lam, order, self_norm, n_live, tag):
    worst, n_val, n_inf = 0.0, 0, 0
    lam32 = float(np.float32(lam))
    for r in range(y.shape[0]):
        if r >= n_live:
            assert same_bits(y2[r], y[r]), (tag, r)
            continue
        assert same_bits(y2[r, V:], y[r, V:]), (tag, r)                     # the padding: the same bits
        h = context_in_use(hist[r], order)
        q = table.logq_all(h, V)
        want = mixed_logits(table, h, y[r, :V], lam32, bool(self_norm))
        back = sum((table.entry(h[i:]) or (0.0, 0.0))[1] for i in range(len(h)))
        bar = y_bar(y[r, :V], q, back, lam, self_norm, want)
        at = np.isfinite(q)
        assert same_bits(y2[r, :V][~at], y[r, :V][~at]), (tag, r)          # q = -inf: the same bits
        err = np.abs(y2[r, :V].astype(np.float64) - want)[at]
        assert np.all(err <= bar[at]), (tag, r, hist[r].tolist(), float((err / bar[at]).max()))
        if at.any():
            worst = max(worst, float((err / bar[at]).max()))
        n_val += int(at.sum())
        n_inf += int((~at).sum())
    print("%s: %d patched words, %d with q = -inf, max err / bar %.3f" % (tag, n_val, n_inf, worst))
    return worst


TABLES = {}


def table_for(V):
    if V not in TABLES:
        n_bi, n_tri = {5: (8, 6), 157: (400, 500), 2003: (3000, 4000)}[V]
        full = {5: (2, 3), 157: (7, 11), 2003: None}[V]
        TABLES[V] = make_table(V, 100 + V, n_bi, n_tri, full_ctx=full)
    return TABLES[V]


@pytest.mark.parametrize("self_norm", [0, 1])
@pytest.mark.parametrize("lam", [0.1, 0.5])
@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("V,R", [(5, 1), (5, 17), (157, 3), (157, 17), (2003, 1), (2003, 3), (2003, 17)])
def test_shapes(V, R, order, lam, self_norm):
    table = table_for(V)
    arr = table.successor_arrays(V)
    hs = histories(table, V, arr)
    if V == 5:
        hs["a list that covers every word"] = (2, 3)
    elif V == 157:
        hs["a list that covers every word"] = (7, 11)
        assert arr["max_probe"] >= 1 and any(k.startswith("displacement") for k in hs)
    names = sorted(hs)
    if V >= 157:
        assert {"none", "trigram context with bow(u v)", "trigram context without bow(u v)", "bigram only, bow(v) != 0",
                "bow(u v) and no trigram successor", "no context (u, v)", "no successor of v at all", "v without a unigram",
                "bigram only, bow(v) = 0"} <= set(names), names
    for start in range(0, len(names), R):                                  # every history of the list, R rows a launch
        hist = np.array([hs[names[(start + i) % len(names)]] for i in range(R)], dtype=np.int32)
        y = make_rows(V, R, 7 * V + R + start)
        y[0, V // 2] = -np.inf                                             # the model gives the word no mass
        rc, y2, flags = launch(table, V, y, hist, lam, order, self_norm)
        assert rc == 0 and flags == 0, (rc, flags)
        check_rows(table, V, y, hist, y2, lam, order, self_norm, R, "V %d R %d order %d lam %g sn %d @%d" % (V, R, order, lam, self_norm, start))
        q0 = table.logq_all(context_in_use(hist[0], order), V)
        assert np.isfinite(y2[0, V // 2]) == bool(np.isfinite(q0[V // 2]))
        rc, y3, _ = launch(table, V, y, hist, lam, order, self_norm)
        assert rc == 0 and same_bits(y2, y3)                               # two launches: the same bits


def test_a_row_alone_inside_a_batch_and_under_a_live_count():
    """the bytes of a row are a function of its logits, its history and the table: the same alone as among seventeen, whatever the
    other rows and the padding hold; rows past the host bound or the device-side live count keep every byte"""
    V, R = 2003, 17
    table = table_for(V)
    hs = list(histories(table, V, table.successor_arrays(V)).values())
    hist = np.array([hs[i % len(hs)] for i in range(R)], dtype=np.int32)
    y = make_rows(V, R, 5)
    rc, full, flags = launch(table, V, y, hist, 0.5, 3)
    assert rc == 0 and flags == 0
    for r in (0, 5, 16):
        one = make_rows(V, 1, 99)
        one[0, :V] = y[r, :V]
        one[0, V:] = 7.0                                                   # another padding
        rc, y1, _ = launch(table, V, one, hist[r:r + 1], 0.5, 3)
        assert rc == 0 and same_bits(y1[0, :V], full[r, :V]) and np.all(y1[0, V:] == 7.0), r
    for live, n_dev in ((17, 11), (9, None), (17, 0), (12, 40)):
        rc, part, flags = launch(table, V, y, hist, 0.5, 3, live=live, n_dev=n_dev)
        n = min(live, live if n_dev is None else n_dev)
        assert rc == 0 and flags == 0 and same_bits(part[:n], full[:n]) and same_bits(part[n:], y[n:]), (live, n_dev)
        check_rows(table, V, y, hist, part, 0.5, 3, 0, n, "live %s / %s" % (live, n_dev))


def test_flags_leave_the_row_as_it_is():
    """a +inf or NaN logit (L not finite): bit 2; a history id outside [-1, V): bit 4; the row keeps every byte and the other rows
    are the bits of a clean launch.  On a self-normalised model L = 0 whatever the row holds: no bit 2."""
    V, R = 157, 4
    table = table_for(V)
    hist = np.array([(7, 11), (-1, 3), (2, 5), (-1, -1)], dtype=np.int32)
    y = make_rows(V, R, 3)
    rc, clean, flags = launch(table, V, y, hist, 0.5, 3)
    assert rc == 0 and flags == 0
    for bad in (np.inf, np.nan):
        yb = y.copy()
        yb[1, 9] = bad
        rc, y2, flags = launch(table, V, yb, hist, 0.5, 3)
        assert rc == 0 and flags == 2 and same_bits(y2[1], yb[1]) and same_bits(np.delete(y2, 1, 0), np.delete(clean, 1, 0))
    yb = y.copy()
    yb[2, :V] = -np.inf
    rc, y2, flags = launch(table, V, yb, hist, 0.5, 3)
    assert rc == 0 and flags == 2 and same_bits(y2[2], yb[2])
    for bad in ((V, 3), (3, V), (-2, 3), (3, -2), (1 << 30, 0)):
        hb = hist.copy()
        hb[2] = bad
        rc, y2, flags = launch(table, V, y, hb, 0.5, 3)
        assert rc == 0 and flags == 4 and same_bits(y2[2], y[2]) and same_bits(np.delete(y2, 2, 0), np.delete(clean, 2, 0)), bad
    # (u, -1) is "no history": u is not looked at beyond its range
    hb = hist.copy()
    hb[0] = (5, -1)
    rc, y2, flags = launch(table, V, y, hb, 0.5, 3)
    assert rc == 0 and flags == 0
    check_rows(table, V, y, hb, y2, 0.5, 3, 0, R, "(u, -1)")


def test_table_indices_are_checked_before_use():
    """ranges and words that point outside the arrays are skipped, whatever the table holds: a launch whose lengths say the lists are
    empty patches from the unigrams alone -- the order-1 result with the back-off weights of the contexts"""
    V = 157
    table = table_for(V)
    hist = np.array([(7, 11), (-1, 3), (2, 5)], dtype=np.int32)
    y = make_rows(V, 3, 8)
    rc, y2, flags = launch(table, V, y, hist, 0.5, 3, struct_over=dict(n_bi=0, n_tri=0))
    assert rc == 0 and flags == 0
    # every range now ends beyond its (declared) list: both successor passes are skipped, every word with a unigram is patched
    lam32 = float(np.float32(0.5))
    for r in range(3):
        assert same_bits(y2[r, V:], y[r, V:])
        h = context_in_use(hist[r], 3)
        back = sum((table.entry(h[i:]) or (0.0, 0.0))[1] for i in range(len(h)))
        q = table.logq_all([], V) + back
        at = np.isfinite(q)
        yr = y[r, :V].astype(np.float64)
        want = yr.copy()
        want[at] = np.logaddexp(yr[at], np.log(np.exp(yr).sum()) + np.log(lam32) - np.log1p(-lam32) + q[at])
        assert same_bits(y2[r, :V][~at], y[r, :V][~at])
        assert np.all(np.abs(y2[r, :V].astype(np.float64) - want)[at] <= y_bar(yr, q, back, 0.5, 0, want)[at]), r


def test_refusals_launch_nothing():
    V = 157
    table = table_for(V)
    tens, arr = successor_tensors(table, V, dev())
    y = make_rows(V, 2, 1)
    ld = y.shape[1]
    yd = torch.from_numpy(y).to(dev())
    hd = torch.tensor([[7, 11], [-1, 3]], device=dev(), dtype=torch.int32)
    flags = torch.zeros(1, device=dev(), dtype=torch.int32)
    lib = _lib.lib()
    names = ["y", "ld_y", "n_cols", "self_norm", "table", "hist", "n_rows", "n_dev", "lam", "order", "flags", "stream"]

    def call(struct=None, **kw):
        t = rows_struct(tens, arr, **(struct or {}))
        a = [yd.data_ptr(), ld, V, 0, ctypes.byref(t), hd.data_ptr(), 2, None, 0.5, 3, flags.data_ptr(), None]
        for k, v in kw.items():
            a[names.index(k)] = v
        rc = lib.jlm_ngram_mix_rows(*a)
        twin = lib.jlm_ngram_mix_refuse(*[a[names.index(k)] for k in ("y", "ld_y", "n_cols", "table", "hist", "n_rows", "n_dev", "lam",
                                                                      "order", "flags")])
        assert (rc == -1) == (twin == -1), (struct, kw, rc, twin)
        return rc

    for kw in (dict(order=0), dict(order=4), dict(lam=0.0), dict(lam=1.0), dict(lam=-0.5), dict(lam=float("nan")), dict(y=None),
               dict(y=yd.data_ptr() + 4), dict(hist=None), dict(hist=hd.data_ptr() + 2), dict(n_dev=flags.data_ptr() + 1),
               dict(flags=flags.data_ptr() + 2), dict(n_rows=-1), dict(ld_y=V), dict(ld_y=ld + 1), dict(ld_y=V - 1), dict(n_cols=0),
               dict(n_cols=393217, ld_y=393220), dict(table=None)):
        assert call(**kw) == -1, kw
    for st in (dict(n_bi=-1), dict(n_tri=-1), dict(n_ctx=-1), dict(log2cap=5), dict(log2cap=32), dict(max_probe=-1),
               dict(max_probe=1 << arr["log2cap"]), dict(uni_lp=None), dict(uni_bow=None), dict(bi_off=None), dict(bi_w=None),
               dict(bi_lp=None), dict(tri_off=None), dict(tri_w=None), dict(tri_lp=None), dict(tri_bow=None), dict(ctx_keys=None),
               dict(ctx_vals=None), dict(ctx_keys=tens["ctx_keys"].data_ptr() + 4), dict(uni_lp=tens["uni_lp"].data_ptr() + 2)):
        assert call(struct=st) == -1, st
    assert call(n_rows=0) == 0 and call(n_rows=0, y=None, hist=None) == 0
    torch.cuda.synchronize()
    assert same_bits(yd.cpu().numpy(), y) and int(flags.cpu()[0]) == 0
    # the largest vocabulary the bitmap holds is accepted (the twin alone: nothing of that size is allocated), and 2^18
    t = rows_struct(tens, arr)
    for big in (262144, 393216):
        assert lib.jlm_ngram_mix_refuse(yd.data_ptr(), big, big, ctypes.byref(t), hd.data_ptr(), 2, None, 0.5, 3, None) == 0
    assert call() == 0
    torch.cuda.synchronize()
    assert not same_bits(yd.cpu().numpy(), y)


@pytest.mark.parametrize("V,where", LSE_CASES)
def test_L_is_the_topk_kernels_log_normaliser_bit_for_bit(V, where):
    """tests/row_lse_pin.py: one live row whose maximum 0.0f sits in the first or the last non-empty wave span, no history, a table
    whose unigram of w* is 0.0 and y[w*] = -inf -- y'[w*] has the bits of float32(float32(nll) + log rho), nll jlm_topk_rows' own"""
    y, p, ws = pin_row(V, where)
    lp = np.full(V, -1.0)
    lp[ws] = 0.0
    table = NGramTable(np.arange(1, V + 1, dtype=np.int64), lp, np.zeros(V), 1).rounded()
    assert table.successor_arrays(V)["uni_lp"][ws] == 0.0
    row = make_rows(V, 1, 0)
    row[0, :V] = y
    rc, y2, flags = launch(table, V, row, np.array([(-1, -1)], dtype=np.int32), LSE_LAM, 3)
    assert rc == 0 and flags == 0, (rc, flags)
    got, want = int(y2[0, ws:ws + 1].view(np.uint32)[0]), expected_bits(V, where)
    print("V %d, p = %d (%s span), w* = %d: y'[w*] bits %08x, float32(float32(nll) + log rho) bits %08x" % (V, p, where, ws, got, want))
    assert got == want, (V, where, hex(got), hex(want))
    assert same_bits(y2[0, V:], row[0, V:])


@pytest.mark.parametrize("V", [262144, 393216])
def test_the_largest_vocabularies_run(V):
    """V = 2^18 = 262 144, a 32 KB bitmap, and V = JLM_NGRAM_MIX_MAX_V = 393 216, 48 KB of bitmap beside the kernel's static LDS: one
    row, unigrams alone and a short bigram list, against the definition"""
    rng = np.random.RandomState(4)
    lp = -rng.uniform(0.1, 14.0, size=V)
    keys = np.arange(1, V + 1, dtype=np.int64)
    bi = [pack((V - 1, w)) for w in (0, 31, 32, V - 1)]
    table = NGramTable(np.concatenate([keys, bi]), np.concatenate([lp, [-1.0, -2.0, -0.5, -3.0]]),
                       np.concatenate([np.where(np.arange(V) % 2, -0.25, 0.0), np.zeros(4)]), 2).rounded()
    y = make_rows(V, 1, 2)
    hist = np.array([(-1, V - 1)], dtype=np.int32)
    rc, y2, flags = launch(table, V, y, hist, 0.5, 2)
    assert rc == 0 and flags == 0
    check_rows(table, V, y, hist, y2, 0.5, 2, 0, 1, "V = %d" % V)


def test_hist_advance_against_numpy():
    rng = np.random.RandomState(6)
    for n_in, n in ((1, 1), (5, 17), (300, 300), (17, 1000)):
        hin = rng.randint(-1, 50, size=(n_in, 2)).astype(np.int32)
        prev = rng.randint(0, n_in, size=n).astype(np.int32)
        word = rng.randint(0, 50, size=n).astype(np.int32)
        if n > 3:
            prev[1], prev[2] = -1, n_in                                     # outside the rows: no word before this one
        want = np.stack([np.where((prev >= 0) & (prev < n_in), hin[np.clip(prev, 0, n_in - 1), 1], -1), word], axis=1).astype(np.int32)
        up = lambda a: torch.from_numpy(a).to(dev())
        hd, pd, wd = up(hin), up(prev), up(word)
        out = torch.full((n + 3, 2), -77, device=dev(), dtype=torch.int32)
        lib = _lib.lib()
        assert lib.jlm_ngram_hist_advance(hd.data_ptr(), n_in, pd.data_ptr(), wd.data_ptr(), n, out.data_ptr(), None) == 0
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert np.array_equal(got[:n], want) and np.all(got[n:] == -77), (n_in, n)
        assert same_bits(hd.cpu().numpy(), hin)
        for bad in (dict(n=-1), dict(n_in=-1), dict(hist_in=None), dict(prev_row=None), dict(word=None), dict(hist_out=None),
                    dict(hist_out=hd.data_ptr()), dict(hist_in=hd.data_ptr() + 4), dict(word=wd.data_ptr() + 1)):
            a = dict(hist_in=hd.data_ptr(), n_in=n_in, prev_row=pd.data_ptr(), word=wd.data_ptr(), n=n, hist_out=out.data_ptr())
            a.update(bad)
            assert lib.jlm_ngram_hist_advance(a["hist_in"], a["n_in"], a["prev_row"], a["word"], a["n"], a["hist_out"], None) == -1, bad
    assert _lib.lib().jlm_ngram_hist_advance(None, 0, None, None, 0, None, None) == 0
