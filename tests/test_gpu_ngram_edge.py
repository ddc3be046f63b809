"""GPU: ngram_cell_patch_kernel as jlm_ngram_cell_patch launches it (csrc/jlm_ngram_edge.hip, include/jlm_hip.h), on cells, tables,
back-pointer chains and normaliser slices the test writes -- no model.

Every rewritten edge logit within decode_ngram_budget.edge_bar of the float64 definition (NGramTable.logq; each test prints its
measured share of the bar), everything outside the live (position, slot) pairs bit-unchanged, the folded log-normalisers bit-equal to
what jlm_beam_step's fused fold writes from the same slices, a log-normaliser that is not finite flagged and replaced, a cell alone
the bits it gives among the others, and every launcher refusal -1 without a launch."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
from jlm_amd import _lib                                                                  # noqa: E402
from jlm_amd.ngram import NGramTable, pack                                                # noqa: E402
from tests.decode_ngram_budget import edge_bar                                            # noqa: E402

pytestmark = pytest.mark.gpu

EOS = 1
LAM = 0.3
POISON_WORD = 3                         # what a root row's own word holds: an id every table knows -- reading it would show


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def up(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev())


def make_table(kind, seed):
    """-> (NGramTable of order 3, device_arrays() keywords)"""
    rng = np.random.RandomState(seed)
    grams = []
    if kind == "a":                                                        # every trigram over six words present
        ids = range(6)
        grams = [(w,) for w in ids] + [(v, w) for v in ids for w in ids] + [(u, v, w) for u in ids for v in ids for w in ids]
    elif kind == "b":                                                      # unigrams only: every context weight absent
        grams = [(w,) for w in range(10)]
    elif kind == "c":                                                      # words 5 .. 9 without a unigram
        ids = range(5)
        grams = [(w,) for w in ids] + [(v, w) for v in ids for w in ids if rng.rand() < 0.5] + \
                [(u, v, w) for u in ids for v in ids for w in ids if rng.rand() < 0.5]
    else:                                                                  # sparse, at a load above 0.5: probes walk.  Word 9 is in no
        ids = range(9)                                                     # n-gram, word 8 has no unigram
        grams = [(w,) for w in range(8)] + [(v, w) for v in ids for w in ids if rng.rand() < 0.5] + \
                [(u, v, w) for u in ids for v in ids for w in ids if rng.rand() < 0.3]
    lp = -rng.uniform(0.05, 9.0, size=len(grams)).astype(np.float32)
    bow = np.where([len(g) < 3 and kind != "b" for g in grams], rng.uniform(-3.0, 0.5, size=len(grams)), 0.0).astype(np.float32)
    table = NGramTable([pack(g) for g in grams], lp, bow, 3)
    kw = dict(log2cap=max(6, int(np.ceil(np.log2(1.3 * len(grams)))))) if kind == "d" else {}
    return table, kw


def of_order(table, order):
    keep = table.keys < (1 << (21 * order))
    return NGramTable(table.keys[keep], table.lp[keep], table.bow[keep], order)


class Cells:
    """seven cells of one frame over pools of 24 older rows: roots (0 .. 7), rows whose parent is a root (8 .. 15), deeper rows"""

    def __init__(self, beam, seed, force=None):
        rng = np.random.RandomState(seed)
        self.beam, self.B, self.frame = beam, 7, 1
        B = self.B
        self.cnt = np.array([beam, max(beam - 1, 1), beam, 0, 1, beam, beam], dtype=np.int32)
        self.sent_len = np.array([3, 3, 3, 3, 3, 1, 3], dtype=np.int32)   # sentence 5 is past its end at frame 1
        self.root_hist = np.array([[-1, EOS], [4, 2], [-1, EOS], [0, 5], [2, 2], [1, 1], [7, EOS]], dtype=np.int32)
        old = 24
        G = old + B * beam
        self.bp = np.full(G, -1, dtype=np.int32)
        self.word = np.full(G, POISON_WORD, dtype=np.int32)
        self.bp[8:16], self.word[8:16] = rng.randint(0, 8, size=8), rng.randint(0, 10, size=8)
        self.bp[16:24], self.word[16:24] = rng.randint(8, 16, size=8), rng.randint(0, 10, size=8)
        kinds = rng.randint(0, 4, size=B * beam)                           # a root | its parent a root | deeper (twice as often)
        self.bp[old:] = np.where(kinds == 0, -1, np.where(kinds == 1, rng.randint(0, 8, size=B * beam), rng.randint(8, 24, size=B * beam)))
        self.word[old:] = np.where(kinds == 0, POISON_WORD, rng.randint(0, 10, size=B * beam))
        self.g0 = (old + np.arange(B) * beam).astype(np.int32)
        self.score = rng.uniform(0.0, 30.0, size=G)
        J = [1, 40, 5, 5, 40, 5, 3]
        lists = [rng.randint(0, 12, size=n).astype(np.int32) for n in J]    # duplicates on different nodes; 10, 11: in no table
        lists[1][:3] = (0, 0, 400)
        if force is not None:                                              # this n-gram is looked up: slot 0 of cell 0, position 0
            g = self.g0[0]
            lists[0][0] = force[-1]
            self.bp[g], self.word[g] = 16, (force[-2] if len(force) >= 2 else 9)
            self.word[16] = force[-3] if len(force) == 3 else 9            # (9: in no n-gram of table d, so a bigram is walked to)
        self.wl = np.concatenate(lists)
        self.wl_off = np.concatenate(([0], np.cumsum(J))).astype(np.int32)
        self.wl_out = rng.permutation(len(self.wl)).astype(np.int32)
        self.edge = (3.0 * rng.standard_normal(len(self.wl) * beam) - 6.0).astype(np.float32)
        self.n_parts = 7
        self.part = np.stack([5.0 * rng.standard_normal((self.n_parts, B * beam)), rng.uniform(1.0, 50.0, size=(self.n_parts, B * beam))],
                             axis=-1).astype(np.float32)
        self.live_base = (np.array([0, 2, 1, 3, 4, 5, 6]) * beam).astype(np.int32)

    def history(self, j, k):
        g = self.g0[j] + k
        b = self.bp[g]
        if b < 0:
            h = self.root_hist[j]
        else:
            h = (self.root_hist[j][1] if self.bp[b] < 0 else self.word[b], self.word[g])
        return [int(x) for x in h if x >= 0]


def patch(arr, C, order, lam=LAM, self_norm=False, only=None, score=True, **over):
    """-> (rc, edge', lse [B * beam], flags); only: the one cell launched"""
    sel = slice(None) if only is None else slice(only, only + 1)
    B = C.B if only is None else 1
    keep = dict(keys=up(arr["keys"].view(np.int64), np.int64), vals=up(arr["vals"], np.float32), g0=up(C.g0[sel], np.int32),
                cnt=up(C.cnt[sel], np.int32), sent_len=up(C.sent_len[sel], np.int32), bp=up(C.bp, np.int32), word=up(C.word, np.int32),
                score=up(C.score, np.float64), root_hist=up(C.root_hist[sel], np.int32), wl=up(C.wl, np.int32),
                wl_off=up(C.wl_off, np.int32), wl_idx=up(np.arange(C.B)[sel], np.int32), wl_out=up(C.wl_out, np.int32),
                part=up(C.part, np.float32), live_base=up(C.live_base[sel], np.int32))
    ed = up(C.edge, np.float32)
    lse = torch.full((C.B * C.beam,), -7.0, device=dev(), dtype=torch.float64)
    flags = torch.zeros(1, device=dev(), dtype=torch.int32)
    a = dict(keys=keep["keys"].data_ptr(), vals=keep["vals"].data_ptr(), log2cap=arr["log2cap"], max_probe=arr["max_probe"], order=order,
             lam=lam, beam=C.beam, part=None if self_norm else keep["part"].data_ptr(), n_parts=0 if self_norm else C.n_parts,
             live_base=keep["live_base"].data_ptr(), lse=lse.data_ptr(), edge=ed.data_ptr(), root_hist=keep["root_hist"].data_ptr(),
             score=keep["score"].data_ptr() if score else None)
    a.update(over)
    torch.cuda.synchronize()
    rc = _lib.lib().jlm_ngram_cell_patch(a["keys"], a["vals"], a["log2cap"], a["max_probe"], a["order"], a["lam"], keep["g0"].data_ptr(),
                                         keep["cnt"].data_ptr(), keep["sent_len"].data_ptr(), C.frame, B, a["beam"], keep["bp"].data_ptr(),
                                         keep["word"].data_ptr(), a["score"], a["root_hist"], keep["wl"].data_ptr(),
                                         keep["wl_off"].data_ptr(), keep["wl_idx"].data_ptr(), 0, keep["wl_out"].data_ptr(), a["edge"],
                                         a["part"], C.B * C.beam, a["n_parts"], a["live_base"], a["lse"], flags.data_ptr(), None)
    torch.cuda.synchronize()
    return rc, ed.cpu().numpy(), lse.cpu().numpy(), int(flags.cpu()[0])


def fold64(part, base, k):
    m = part[:, base + k, 0].astype(np.float64)
    sm = part[:, base + k, 1].astype(np.float64)
    top = m.max()
    return top + np.log((sm * np.exp(m - top)).sum())


def displaced_entry(table, arr):
    """the ids of an entry that sits max_probe slots behind its home"""
    cap = 1 << arr["log2cap"]
    keys = arr["keys"]
    at = np.nonzero(keys)[0]
    home = ((keys[at] * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(64 - arr["log2cap"])).astype(np.int64)
    disp = (at - home) % cap
    assert int(disp.max()) == arr["max_probe"]
    key = int(keys[at[int(np.argmax(disp))]])
    ids = [((key >> sh) & 0x1FFFFF) - 1 for sh in (42, 21, 0)]
    return tuple(x for x in ids if x >= 0)


def check(C, table, arr, order, self_norm, tag):
    """one launch against the definition -> the largest share of the bar"""
    rc, e2, lse, flags = patch(arr, C, order, self_norm=self_norm)
    assert rc == 0 and flags == 0, tag
    ref_table = of_order(table, order)
    lamf = float(np.float32(LAM))
    log1m, log_rho = np.log1p(-lamf), np.log(lamf) - np.log1p(-lamf)
    beam = C.beam
    got = e2.reshape(len(C.wl), beam)
    want_same = C.edge.copy().reshape(len(C.wl), beam)
    worst = 0.0
    for j in range(C.B):
        live = C.frame < C.sent_len[j]
        for k in range(beam):
            g = j * beam + k
            if live and k < C.cnt[j] and not self_norm:
                L = fold64(C.part, C.live_base[j], k)
                assert abs(lse[g] - L) <= 1e-6 * (1 + abs(L)), (tag, j, k, lse[g], L)         # (f32 expf inside the fold)
            else:
                assert lse[g] == -7.0, (tag, j, k)
        if not live:
            continue
        for k in range(C.cnt[j]):
            h = C.history(j, k)
            L = 0.0 if self_norm else float(lse[j * beam + k])             # (the fold's own value: its error is not the patch's)
            for p in range(C.wl_off[j], C.wl_off[j + 1]):
                y = float(C.edge[C.wl_out[p] * beam + k])
                q = ref_table.logq(h, int(C.wl[p]))
                ref = L + log1m + np.logaddexp(y - L, log_rho + q) if np.isfinite(q) else y + log1m
                bar = edge_bar(ref)
                err = abs(float(got[C.wl_out[p], k]) - ref)
                worst = max(worst, err / bar)
                assert err <= bar, (tag, j, k, p, h, int(C.wl[p]), got[C.wl_out[p], k], ref, bar)
                want_same[C.wl_out[p], k] = got[C.wl_out[p], k]
    # everything else -- a sentence past its end, slots past cnt -- keeps the bits of the buffer
    assert got.tobytes() == want_same.tobytes(), tag
    return worst


@pytest.mark.parametrize("kind", ["a", "b", "c", "d"])
@pytest.mark.parametrize("beam", [1, 3, 17, 20])
def test_patch_against_the_definition(beam, kind):
    table, kw = make_table(kind, seed=11)
    arr = table.device_arrays(**kw)
    force = None
    if kind == "d":
        assert arr["max_probe"] >= 3 and 2 * len(table) >= (1 << arr["log2cap"])
        force = displaced_entry(table, arr)
    C = Cells(beam, seed=100 * beam + ord(kind), force=force)
    if force is not None:                                                  # the look-up that ends max_probe slots behind its home happens
        h = C.history(0, 0)
        assert tuple(h[len(h) - (len(force) - 1):] if len(force) > 1 else ()) == force[:-1] and C.wl[0] == force[-1]
    worst = 0.0
    for order in (1, 2, 3):
        for self_norm in (0, 1):
            worst = max(worst, check(C, table, arr, order, self_norm, (beam, kind, order, self_norm)))
    # a cell alone gives the bits it gives among the others
    j = 2
    _rc, all_, _l, _f = patch(arr, C, 3)
    rc, alone, _l, _f = patch(arr, C, 3, only=j)
    nodes = C.wl_out[C.wl_off[j]:C.wl_off[j + 1]]
    assert rc == 0 and alone.reshape(-1, beam)[nodes].tobytes() == all_.reshape(-1, beam)[nodes].tobytes()
    rest = np.setdiff1d(np.arange(len(C.wl)), nodes)
    assert alone.reshape(-1, beam)[rest].tobytes() == C.edge.reshape(-1, beam)[rest].tobytes()
    print("ngram patch beam=%d table=%s: largest share of the edge bar %.3f" % (beam, kind, worst))


def test_the_histories_of_all_four_kinds_occur():
    C = Cells(17, seed=5)
    seen = set()
    for j in range(C.B):
        for k in range(C.cnt[j]):
            g = C.g0[j] + k
            b = C.bp[g]
            seen.add(("root", int(C.root_hist[j][0] >= 0)) if b < 0 else ("parent is a root", int(C.root_hist[j][0] >= 0))
                     if C.bp[b] < 0 else ("deeper", 0))
    assert {("root", 0), ("root", 1), ("parent is a root", 1), ("deeper", 0)} <= seen


def test_a_slot_whose_score_is_not_finite_keeps_its_logits():
    table, kw = make_table("a", seed=11)
    arr = table.device_arrays(**kw)
    C = Cells(3, seed=9)
    _rc, base, _l, _f = patch(arr, C, 3)
    C.score[C.g0[0] + 1] = np.inf
    rc, e2, _l, flags = patch(arr, C, 3)
    assert rc == 0 and flags == 8
    beam = C.beam
    nodes = C.wl_out[C.wl_off[0]:C.wl_off[1]]
    got, before = e2.reshape(-1, beam), C.edge.reshape(-1, beam)
    assert got[nodes, 1].tobytes() == before[nodes, 1].tobytes()
    keep = np.ones_like(got, dtype=bool)
    keep[nodes, 1] = False
    assert got[keep].tobytes() == base.reshape(-1, beam)[keep].tobytes()
    # without the score pool nothing is looked at
    rc, e3, _l, flags = patch(arr, C, 3, score=False)
    assert rc == 0 and flags == 0 and e3.tobytes() == base.tobytes()


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
    slices = np.zeros((n_parts, G, 2), np.float32)
    slices[:, :, 0] = rng.uniform(-5.0, 15.0, size=(n_parts, G)).astype(np.float32)
    slices[:, :, 1] = np.exp(rng.uniform(0.0, np.log(1.0e4), size=(n_parts, G))).astype(np.float32)
    _lse0, edge = dyadic_inputs(P, 3)
    S = State(P, np.full(G, 1.0e30), edge, True)
    mine = torch.full((G,), -7.0, device=dev(), dtype=torch.float64)
    table, _kw = make_table("b", seed=1)
    arr = table.device_arrays()
    keys, vals = up(arr["keys"].view(np.int64), np.int64), up(arr["vals"], np.float32)
    idx = up(np.arange(B), np.int32)
    zeros = torch.zeros(8, device=dev(), dtype=torch.int32)
    lists = torch.zeros(B + 1, device=dev(), dtype=torch.int32)           # every list empty: the patch folds and touches nothing else
    root = up(np.tile([-1, EOS], (B, 1)), np.int32)
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
        pn[:, :nl] = slices[:, lv]
        part.copy_(up(pn, np.float32))
        edge_before = S.edge.clone()
        g0 = up(f * rmax + np.arange(B) * beam, np.int32)
        rc = lib.jlm_ngram_cell_patch(keys.data_ptr(), vals.data_ptr(), arr["log2cap"], arr["max_probe"], 3, 0.25, g0.data_ptr(),
                                      S.cnt.data_ptr() + 4 * f * B, S.ints["slen"].data_ptr(), f, B, beam, S.bp.data_ptr(),
                                      S.word.data_ptr(), S.score.data_ptr(), root.data_ptr(), zeros.data_ptr(), lists.data_ptr(),
                                      idx.data_ptr(), 0, zeros.data_ptr(), S.edge.data_ptr(), part.data_ptr(), rmax, n_parts,
                                      S.live_base.data_ptr() + 4 * f * B, mine.data_ptr() + 8 * f * rmax, S.flags.data_ptr(), _stream())
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
    table, kw = make_table("a", seed=11)
    arr = table.device_arrays(**kw)
    C = Cells(3, seed=4)
    C.part[0, C.live_base[0] + 1] = (0.0, np.inf)
    rc, e2, lse, flags = patch(arr, C, 3)
    assert rc == 0 and flags == 1 and lse[1] == 1.0e30
    live = lse != -7.0
    assert np.isfinite(lse[live]).all() and np.isfinite(e2).all()


def test_refusals_launch_nothing():
    table, kw = make_table("a", seed=11)
    arr = table.device_arrays(**kw)
    C = Cells(3, seed=4)
    ok = patch(arr, C, 3)
    assert ok[0] == 0 and ok[1].tobytes() != C.edge.tobytes()
    bad = [dict(order=0), dict(order=4), dict(log2cap=5), dict(log2cap=32), dict(max_probe=1 << arr["log2cap"]), dict(max_probe=-1),
           dict(lam=0.0), dict(lam=1.0), dict(lam=float("nan")), dict(beam=0), dict(beam=1025), dict(keys=None), dict(vals=None),
           dict(edge=None), dict(root_hist=None), dict(live_base=None), dict(lse=None), dict(n_parts=0)]
    for over in bad:
        kw = dict(over)
        rc, e2, lse, flags = patch(arr, C, kw.pop("order", 3), lam=kw.pop("lam", LAM), **kw)
        assert rc == -1 and flags == 0 and e2.tobytes() == C.edge.tobytes() and (lse == -7.0).all(), over
    # a misaligned pointer
    keys = up(np.concatenate((arr["keys"], arr["keys"][:1])).view(np.int64), np.int64)
    rc, e2, _l, _f = patch(arr, C, 3, keys=keys.data_ptr() + 4)
    assert rc == -1 and e2.tobytes() == C.edge.tobytes()
