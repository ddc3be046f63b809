"""GPU: jlm_alt_head (csrc/jlm_alt.hip) through its C entry point on synthetic pools, lattice-free: the test writes the pools, the
back-pointer chains and the rows itself, as tests/test_gpu_tail_predict.py does.

Expected values: head = score + lse - edge in float64 with ``edge`` from jlm_edge_logits on the same rows and words -- bit for bit --,
the accumulator seed and prev0 from a host walk of bp, the copied state rows byte for byte.  The scores along a path are built as
score[g_k] = score[g_{k-1}] + lse[g_{k-1}] - edge(own word), so the own word's head must equal score[g_k] to the bit.

Models: one segment of k = 32 and of k = 512 (the k > 256 tail of the dot product), two segments (32 + 20, 200 + 100).  Beams 1, 3, 17
and 65, rank 0 and beam - 1; paths of one segment and of n_frames - 1 one-kana segments (19: a second 16-row pass); 1, 63, 64, 65 and
300 alternatives in a segment; a sentence without rows; state rows as random bit patterns (any row format) and as f32; mode 1; a NaN
log-normaliser, broken chains, poison around and inside every output, a second problem on the first one's buffers, every refusal."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
from jlm_amd import _lib                                                         # noqa: E402
from tests import poison                                                         # noqa: E402

pytestmark = pytest.mark.gpu

V = 1500
MODELS = {"k32": [32], "k512": [512], "k32+20": [32, 20], "k200+100": [200, 100]}
GUARD = 5


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return _lib.lib()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _g(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


class Problem:
    """random pools of a decode of len(paths) sentences x ``n_frames`` frames at ``beam``.  paths: per sentence the end frames
    e_1 < ... < e_K of its path's segments (sent_len = e_K); alts: per sentence, per segment, how many alternatives (the own word is
    alternative 0; None: the sentence has no rows)."""

    def __init__(self, L, widths, beam, rank, paths, alts, n_frames, H=32, seed=0, f32_state=False, mode=0):
        rng = np.random.default_rng(seed)
        self.beam, self.rank, self.B, self.F, self.H, self.mode = beam, rank, len(paths), n_frames, H, mode
        self.paths, self.alts = paths, alts
        B, F = self.B, n_frames
        self.rmax = B * beam
        G = self.G = F * self.rmax
        cut = np.linspace(0, V, len(widths) + 1).astype(int)
        self.ldt = sum(widths) + 4
        t_off = np.concatenate([[0], np.cumsum(widths)[:-1]]).astype(int)
        self.Bg = [_g((rng.standard_normal((cut[i + 1] - cut[i], k + 4)) * 0.3).astype(np.float32)) for i, k in enumerate(widths)]
        self.segs = (_lib.Segment * len(widths))(*[
            _lib.Segment(int(cut[i]), int(cut[i + 1]), k, int(t_off[i]), self.Bg[i].data_ptr(), k + 4) for i, k in enumerate(widths)])
        self.n_segs = len(widths)
        self.b2 = rng.standard_normal(V).astype(np.float32)
        self.T = (rng.standard_normal((G, self.ldt)) * 0.5).astype(np.float32)
        self.score = rng.uniform(0.0, 30.0, G)
        self.lse = rng.uniform(5.0, 9.0, G) if mode == 0 else np.full(G, np.nan)
        if f32_state:
            self.h, self.c = (rng.standard_normal((G, H)).astype(np.float32).view(np.int32) for _ in range(2))
        else:                                  # any bit pattern: split rows, NaN payloads -- the copy is byte for byte
            self.h, self.c = (rng.integers(-2 ** 31, 2 ** 31 - 1, (G, H)).astype(np.int32) for _ in range(2))
        self.bp = rng.integers(-900, -2, G).astype(np.int32)        # off the chains: nowhere
        self.sent_len = np.array([p[-1] for p in paths], np.int32)
        self.chain, self.words = [], []
        for s, ends in enumerate(paths):
            g = [s * beam]
            self.bp[g[0]] = -1
            for i, e in enumerate(ends):
                slot = rank if i == len(ends) - 1 else int(rng.integers(0, beam))
                g.append(e * self.rmax + s * beam + slot)
                self.bp[g[-1]] = g[-2]
            self.chain.append(g)
            self.words.append([rng.choice(V, size=n, replace=False).astype(np.int32) if n else np.zeros(0, np.int32)
                               for n in (alts[s] or [0] * len(ends))])
        self._edges(L)
        for s, g in enumerate(self.chain):     # the path's scores, as the beam step forms them from the own word's edge
            if alts[s] is None:
                continue
            for k in range(1, len(g)):
                base = self.score[g[k - 1]] + self.lse[g[k - 1]] if mode == 0 else self.score[g[k - 1]]
                self.score[g[k]] = base - float(self.edge[s][k - 1][0])

    def _edges(self, L):
        """jlm_edge_logits over one group per (sentence, segment): row g_{k-1}, the segment's words -> edge[s][k - 1] float32 [words]"""
        groups = [(s, k) for s in range(self.B) for k in range(len(self.paths[s])) if len(self.words[s][k])]
        g0 = np.array([self.chain[s][k] for s, k in groups], np.int32)
        wl = np.concatenate([self.words[s][k] for s, k in groups]).astype(np.int32)
        off = np.zeros(len(groups) + 1, np.int32)
        np.cumsum([len(self.words[s][k]) for s, k in groups], out=off[1:])
        out = torch.full((len(wl) * self.beam,), float("nan"), dtype=torch.float32, device="cuda")
        self.dT, self.db2 = _g(self.T), _g(self.b2)
        a = [_g(x) for x in (g0, np.zeros(len(groups), np.int32), wl, off, np.arange(len(groups), dtype=np.int32),
                             np.arange(len(wl), dtype=np.int32), np.ones(1, np.int32))]
        rc = L.jlm_edge_logits(self.segs, self.n_segs, self.db2.data_ptr(), self.dT.data_ptr(), self.ldt, a[0].data_ptr(), a[6].data_ptr(),
                               a[1].data_ptr(), a[2].data_ptr(), a[3].data_ptr(), a[4].data_ptr(), 0, a[5].data_ptr(), out.data_ptr(),
                               self.beam, len(groups), _st())
        assert rc == 0
        torch.cuda.synchronize()
        e = out.cpu().numpy().reshape(len(wl), self.beam)[:, 0]
        assert not np.isnan(e).any()
        self.edge = [[None] * len(self.paths[s]) for s in range(self.B)]
        for j, (s, k) in enumerate(groups):
            self.edge[s][k] = e[off[j]:off[j + 1]]

    def rows(self, lookahead):
        """the call's rows sorted by suffix steps, longest first: (sentence, depth, alternative, j) and the arrays the launch takes"""
        rows = []
        for s in range(self.B):
            K = len(self.paths[s])
            if self.alts[s] is None:
                continue
            for d in range(K):
                j = K - d - 1 if lookahead is None else min(K - d - 1, lookahead)
                rows += [(s, d, i, j) for i in range(len(self.words[s][d]))]
        order = sorted(range(len(rows)), key=lambda q: -rows[q][3])
        rows = [rows[q] for q in order]
        S = rows[0][3] if rows else 0
        n_live = np.array([sum(1 for r in rows if r[3] > t) for t in range(S)], np.int32)
        sent = np.array([r[0] for r in rows], np.int64)
        off = np.zeros(self.B + 1, np.int32)
        np.cumsum(np.bincount(sent, minlength=self.B), out=off[1:])
        srows = np.argsort(sent, kind="stable").astype(np.int32)
        depth = np.array([r[1] for r in rows], np.int32)
        alt = np.array([self.words[r[0]][r[1]][r[2]] for r in rows], np.int32)
        return rows, S, n_live, off, srows, depth, alt

    def expected(self, rows):
        seq = np.zeros(len(rows))
        for r, (s, d, i, j) in enumerate(rows):
            g = self.chain[s]
            base = self.score[g[d]] + self.lse[g[d]] if self.mode == 0 else self.score[g[d]]
            head = base - np.float64(self.edge[s][d][i])
            seq[r] = head + (self.score[g[-1]] - self.score[g[d + 1 + j]])
        return seq

    def run(self, L, lookahead, out=None, fill=poison.FILL_A, expect_rc=0, rows_override=None):
        """-> (rows, got): the launch over freshly poisoned outputs (``out``: another problem's buffers, poisoned again)"""
        rows, S, n_live, off, srows, depth, alt = rows_override or self.rows(lookahead)
        R, H = len(rows), self.H
        d = self.d = {k: _g(getattr(self, k)) for k in ("score", "lse", "bp", "sent_len", "h", "c")}
        pad = lambda x: _g(np.append(x, 0).astype(np.int32))               # (one entry more: never an empty tensor)
        d.update(off=_g(off), srows=pad(srows), depth=pad(depth), alt=pad(alt), n_live=pad(n_live))
        if out is None:
            out = dict(h0=torch.zeros((R + GUARD, H), dtype=torch.int32, device="cuda"), c0=torch.zeros((R + GUARD, H), dtype=torch.int32, device="cuda"),
                       prev0=torch.zeros(R + GUARD, dtype=torch.int32, device="cuda"), seq=torch.zeros(R + GUARD, dtype=torch.float64, device="cuda"),
                       flags=torch.zeros(1 + GUARD, dtype=torch.int32, device="cuda"))
        for k, t in out.items():
            poison.fill_tensor(t, fill)
        out["flags"][0] = 0
        before = {k: v.clone() for k, v in out.items()}
        a, p = _lib.AltPlan(), _lib.ScorePlan()
        a.n_sent, a.beam, a.n_frames, a.rank = self.B, self.beam, self.F, self.rank
        a.h, a.c, a.T, a.score, a.lse, a.bp = d["h"].data_ptr(), d["c"].data_ptr(), self.dT.data_ptr(), d["score"].data_ptr(), d["lse"].data_ptr(), d["bp"].data_ptr()
        a.sent_len, a.sent_off, a.sent_rows, a.depth, a.alt = d["sent_len"].data_ptr(), d["off"].data_ptr(), d["srows"].data_ptr(), d["depth"].data_ptr(), d["alt"].data_ptr()
        a.prev0 = p.prev0 = out["prev0"].data_ptr()
        p.n_rows, p.n_steps = R, S
        p.h[0], p.c[0], p.n_live, p.nll_seq, p.flags = out["h0"].data_ptr(), out["c0"].data_ptr(), d["n_live"].data_ptr(), out["seq"].data_ptr(), out["flags"].data_ptr()
        self.plans = (a, p)
        rc = L.jlm_alt_head(self.segs, self.n_segs, self.db2.data_ptr(), self.ldt, H, self.mode, a, p, _st())
        assert rc == expect_rc, rc
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in out.items()}
        got["before"] = {k: v.cpu().numpy() for k, v in before.items()}
        got["out"] = out
        return rows, got

    def check(self, L, lookahead, out=None, fill=poison.FILL_A):
        rows, got = self.run(L, lookahead, out, fill)
        R, b = len(rows), got["before"]
        want = self.expected(rows)
        assert got["seq"][:R].tobytes() == want.tobytes(), (got["seq"][:R], want)                        # bit-equal
        assert got["prev0"][:R].tolist() == list(range(R))
        assert got["flags"][0] == 0
        for r, (s, d, i, j) in enumerate(rows):
            g = self.chain[s][d]
            if j >= 1:
                assert got["h0"][r].tobytes() == self.h[g].tobytes() and got["c0"][r].tobytes() == self.c[g].tobytes(), r
            else:                                                                                          # never live: not written
                assert got["h0"][r].tobytes() == b["h0"][r].tobytes() and got["c0"][r].tobytes() == b["c0"][r].tobytes(), r
            if i == 0 and lookahead is None:                                                               # the own word
                assert got["seq"][r] == self.score[self.chain[s][d + 1]], (r, s, d)
        for k in ("h0", "c0", "prev0", "seq"):
            assert got[k][R:].tobytes() == b[k][R:].tobytes(), "wrote past the outputs: " + k
        assert got["flags"][1:].tobytes() == b["flags"][1:].tobytes()
        return rows, got


def standard(F):
    """paths and alternative counts: one segment | F - 1 one-kana segments | 3 segments with 63 / 64 / 65 alternatives | a sentence
    without rows | 2 segments, 300 alternatives in one"""
    paths = [[F - 1], list(range(1, F)), [2, 3, F - 2], [1, F - 1], [3, F - 1]]
    alts = [[1], [2] * (F - 1), [63, 64, 65], None, [300, 5]]
    return paths, alts


@pytest.mark.parametrize("lookahead", [None, 0, 1])
@pytest.mark.parametrize("beam,last", [(1, False), (3, False), (3, True), (17, True), (65, False), (65, True)])
def test_beams_ranks_and_lookaheads(L, beam, last, lookahead):
    F = 20                                                  # 19 one-kana segments: a second pass of 16 staged rows
    paths, alts = standard(F)
    p = Problem(L, MODELS["k32+20"], beam, beam - 1 if last else 0, paths, alts, F, seed=beam + 7 * last)
    rows, _got = p.check(L, lookahead)
    assert len(rows) == 1 + 2 * 19 + 192 + 305
    assert {j for _s, _d, _i, j in rows} == ({0} if lookahead == 0 else {0, 1} if lookahead == 1 else set(range(19)))


@pytest.mark.parametrize("name", ["k32", "k512", "k200+100"])
@pytest.mark.parametrize("f32_state", [False, True], ids=["bits", "f32"])
def test_models_and_state_formats(L, name, f32_state):
    paths, alts = standard(7)
    p = Problem(L, MODELS[name], 3, 1, paths, alts, 7, H=64 if f32_state else 512, seed=11, f32_state=f32_state)
    if len(MODELS[name]) > 1:                               # a segment's alternatives fall in both model segments
        assert {bool(w >= V // 2) for w in p.words[4][0]} == {False, True}
    p.check(L, None)
    p.check(L, 1)


def test_mode_1_reads_no_normaliser(L):
    paths, alts = standard(7)
    p = Problem(L, MODELS["k200+100"], 3, 0, paths, alts, 7, seed=8, mode=1)
    assert np.isnan(p.lse).all()
    p.check(L, None)
    p.d = None
    rows, got = p.run(L, 0)
    a, sp = p.plans
    a.lse = None
    assert L.jlm_alt_head(p.segs, p.n_segs, p.db2.data_ptr(), p.ldt, p.H, 1, a, sp, _st()) == 0
    torch.cuda.synchronize()
    assert got["out"]["seq"].cpu().numpy()[:len(rows)].tobytes() == p.expected(rows).tobytes()


def test_a_second_problem_on_the_first_ones_buffers(L):
    paths, alts = standard(9)
    p = Problem(L, MODELS["k32+20"], 5, 2, paths, alts, 9, seed=3)
    _rows, got = p.check(L, None)
    q = Problem(L, MODELS["k32+20"], 5, 4, paths, alts, 9, seed=4)
    q.check(L, 1, out=got["out"], fill=poison.FILL_B)
    p.check(L, 0, out=got["out"], fill=poison.FILL_A)


def test_nan_lse_sets_the_flag(L):
    paths, alts = standard(7)
    p = Problem(L, MODELS["k32"], 3, 0, paths, alts, 7, seed=5)
    p.lse[p.chain[2][1]] = np.nan
    rows, got = p.run(L, None)
    assert got["flags"][0] == 1
    want = p.expected(rows)
    bad = np.array([s == 2 and d == 1 for s, d, _i, _j in rows])
    assert np.isnan(got["seq"][:len(rows)][bad]).all() and got["seq"][:len(rows)][~bad].tobytes() == want[~bad].tobytes()


@pytest.mark.parametrize("how", ["outside", "negative", "cycle", "short", "length"])
def test_a_broken_chain_gives_inf_and_copies_nothing(L, how):
    paths, alts = standard(7)
    p = Problem(L, MODELS["k32"], 3, 0, paths, alts, 7, seed=6)
    s = 2
    rows_override = None
    if how == "outside":
        p.bp[p.chain[s][2]] = p.G + 3
    elif how == "negative":
        p.bp[p.chain[s][1]] = -5
    elif how == "cycle":
        p.bp[p.chain[s][1]] = p.chain[s][3]
    elif how == "length":
        p.sent_len[s] = 7                                   # a final frame outside the plan
    else:                                                   # rows of a depth the path does not have
        r = list(p.rows(None))
        r[5] = r[5].copy()
        r[5][np.array([x[0] == s for x in r[0]])] += 3
        rows_override = tuple(r)
    rows, got = p.run(L, None, rows_override=rows_override)
    R, b = len(rows), got["before"]
    assert got["flags"][0] == 4
    mine = np.array([x[0] == s for x in rows])
    want = p.expected(rows)
    assert np.isposinf(got["seq"][:R][mine]).all() and (got["prev0"][:R][mine] == -1).all()
    assert got["seq"][:R][~mine].tobytes() == want[~mine].tobytes()
    assert got["prev0"][:R][~mine].tolist() == np.arange(R)[~mine].tolist()
    assert got["h0"][:R][mine].tobytes() == b["h0"][:R][mine].tobytes() and got["c0"][:R][mine].tobytes() == b["c0"][:R][mine].tobytes()
    for k in ("h0", "c0", "prev0", "seq"):
        assert got[k][R:].tobytes() == b[k][R:].tobytes()


def test_a_word_in_no_segment_is_flagged(L):
    paths, alts = standard(7)
    p = Problem(L, MODELS["k32"], 3, 0, paths, alts, 7, seed=12)
    r = list(p.rows(0))
    r[6] = r[6].copy()
    r[6][3] = V + 5
    rows, got = p.run(L, 0, rows_override=tuple(r))
    assert got["flags"][0] == 2 and np.isnan(got["seq"][3])
    keep = np.arange(len(rows)) != 3
    assert got["seq"][:len(rows)][keep].tobytes() == p.expected(rows)[keep].tobytes()


def test_refused_arguments(L):
    paths, alts = standard(7)
    p = Problem(L, MODELS["k32"], 3, 0, paths, alts, 7, seed=9)
    rows, got = p.run(L, 1)
    a0, p0 = p.plans
    seq_before = got["out"]["seq"].clone()

    def call(ldt=p.ldt, H=p.H, mode=0, **kw):
        a, sp = _lib.AltPlan(), _lib.ScorePlan()
        for f, _t in _lib.AltPlan._fields_:
            setattr(a, f, getattr(a0, f))
        for f in ("n_rows", "n_steps", "prev0", "n_live", "nll_seq", "flags"):
            setattr(sp, f, getattr(p0, f))
        sp.h[0], sp.c[0] = p0.h[0], p0.c[0]
        for k, v in kw.items():
            if k in ("h0", "c0"):
                (sp.h if k == "h0" else sp.c)[0] = v
            else:
                setattr(a if hasattr(a, k) and k != "prev0" else sp, k, v)
        rcs = (L.jlm_alt_head_refuse(p.segs, p.n_segs, p.db2.data_ptr(), ldt, H, mode, a, sp),
               L.jlm_alt_head(p.segs, p.n_segs, p.db2.data_ptr(), ldt, H, mode, a, sp, _st()))
        assert rcs[0] == rcs[1] or (rcs[0] == 0 and rcs[1] == 0), rcs
        return rcs[1]
    got["out"]["seq"].fill_(-3.0)
    for kw in (dict(beam=0), dict(beam=1025), dict(rank=3), dict(rank=-1), dict(ldt=p.ldt + 2), dict(H=p.H + 2), dict(mode=2),
               dict(T=None), dict(T=a0.T + 4), dict(h=a0.h + 8), dict(c=None), dict(score=a0.score + 4), dict(lse=None), dict(bp=None),
               dict(sent_len=None), dict(sent_off=None), dict(sent_rows=a0.sent_rows + 2), dict(depth=None), dict(alt=None),
               dict(prev0=None), dict(prev0=p0.prev0 + 4), dict(nll_seq=None), dict(nll_seq=p0.nll_seq + 4), dict(h0=None),
               dict(c0=p0.c[0] + 4), dict(n_live=None), dict(n_frames=0), dict(n_rows=-1), dict(n_steps=-1), dict(ldt=48 * 1024)):
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert (got["out"]["seq"].cpu().numpy() == -3.0).all()                        # -1 comes before any launch
    assert call(n_sent=0) == 0 and call(n_rows=0) == 0
    assert call(lse=None, mode=1) == 0
    assert call() == 0
    torch.cuda.synchronize()
    assert got["out"]["seq"].cpu().numpy()[:len(rows)].tobytes() == seq_before.cpu().numpy()[:len(rows)].tobytes()
