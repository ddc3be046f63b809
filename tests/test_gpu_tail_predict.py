"""GPU: jlm_tail_predict (csrc/jlm_tail.hip) through its C entry point on synthetic beam state.

Expected values: score + lse - edge in float64 with ``edge`` from jlm_edge_logits on the same rows and words -- bit for bit -- in the
order of numpy's stable argsort over the candidates in (span, word, slot) order; traces from a host walk of bp / node.

Models: one segment of k = 32 and of k = 512 (the k > 256 tail of the dot product), two segments (32 + 20, 200 + 100) with ``ids`` a
permutation, so that a span's words fall in both.  Beams 1, 3, 17 (a second 16-row pass) and 65; n_out 1, 10, 64; chunk 64, the
candidate count, one less, and the default with more than 10 000 candidates in one sentence.  Every problem holds a sentence without
spans, a span of one word, a sentence of three spans and one with fewer candidates than n_out; cnt = 1 at frame 0 and below the beam
elsewhere.  Ties (two identical slots), a NaN log-normaliser, mode 1, refused arguments, and guard entries behind every output."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
from jlm_amd import _lib                                                         # noqa: E402

pytestmark = pytest.mark.gpu

V = 1500
MODELS = {"k32": [32], "k512": [512], "k32+20": [32, 20], "k200+100": [200, 100]}
GUARD = 7
I_FILL, F_FILL = -77, -5.5


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return _lib.lib()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _g(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


class Problem:
    """random pools of a decode of ``n_sent`` sentences x ``n_frames`` frames at ``beam``; spans: per sentence [(frame, lo, hi)]"""

    def __init__(self, widths, beam, spans, n_frames=5, seed=0):
        rng = np.random.default_rng(seed)
        self.beam, self.B, self.F, self.spans = beam, len(spans), n_frames, spans
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
        self.ids = rng.permutation(V).astype(np.int32)
        self.score = rng.uniform(0.0, 30.0, G)
        self.lse = rng.uniform(5.0, 9.0, G)
        # cnt = 1 at frame 0, below the beam elsewhere (beam 1: 1)
        self.cnt = np.zeros(F * B, np.int32)
        for f in range(F):
            for s in range(B):
                self.cnt[f * B + s] = 1 if f == 0 else int(rng.integers(1, max(beam, 2)))
        self.bp = np.full(G, -1, np.int32)
        self.node = rng.integers(0, 100000, G).astype(np.int32)
        for f in range(1, F):
            for s in range(B):
                for k in range(beam):
                    pf = int(rng.integers(0, f))
                    self.bp[f * self.rmax + s * beam + k] = pf * self.rmax + s * beam + int(rng.integers(0, self.cnt[pf * B + s]))

    def upload(self):
        self.d = {k: _g(getattr(self, k)) for k in ("b2", "T", "ids", "score", "lse", "cnt", "bp", "node")}
        off = np.zeros(self.B + 1, np.int32)
        np.cumsum([len(s) for s in self.spans], out=off[1:])
        flat = np.array([t for s in self.spans for t in s] + [(0, 0, 0)], np.int32)        # (one entry more: never an empty tensor)
        self.d.update(sp_off=_g(off), sp_frame=_g(flat[:, 0]), sp_lo=_g(flat[:, 1]), sp_hi=_g(flat[:, 2]))

    def edge(self, L):
        """jlm_edge_logits over one group per span -> per span float32 [words, beam]"""
        groups = [(s, f, lo, hi) for s, sp in enumerate(self.spans) for f, lo, hi in sp]
        if not groups:
            return []
        g0 = np.array([f * self.rmax + s * self.beam for s, f, _lo, _hi in groups], np.int32)
        cidx = np.array([f * self.B + s for s, f, _lo, _hi in groups], np.int32)
        wl = np.concatenate([self.ids[lo:hi] for _s, _f, lo, hi in groups]).astype(np.int32)
        off = np.zeros(len(groups) + 1, np.int32)
        np.cumsum([hi - lo for _s, _f, lo, hi in groups], out=off[1:])
        edge = torch.full((len(wl) * self.beam,), float("nan"), dtype=torch.float32, device="cuda")
        a = [_g(x) for x in (g0, cidx, wl, off, np.arange(len(groups), dtype=np.int32), np.arange(len(wl), dtype=np.int32))]
        rc = L.jlm_edge_logits(self.segs, self.n_segs, self.d["b2"].data_ptr(), self.d["T"].data_ptr(), self.ldt, a[0].data_ptr(),
                               self.d["cnt"].data_ptr(), a[1].data_ptr(), a[2].data_ptr(), a[3].data_ptr(), a[4].data_ptr(), 0,
                               a[5].data_ptr(), edge.data_ptr(), self.beam, len(groups), _st())
        assert rc == 0
        torch.cuda.synchronize()
        e = edge.cpu().numpy().reshape(len(wl), self.beam)
        return [e[off[j]:off[j + 1]] for j in range(len(groups))]

    def expected(self, L, n_out, mode=0):
        """per sentence (scores, rows, words) of the n_out best, and its candidate count"""
        edges = self.edge(L)
        out, j = [], 0
        for s, sp in enumerate(self.spans):
            keys, rows, words = [np.zeros(0)], [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
            for f, lo, hi in sp:
                n = min(int(self.cnt[f * self.B + s]), self.beam)
                g0 = f * self.rmax + s * self.beam
                base = self.score[g0:g0 + n] + self.lse[g0:g0 + n] if mode == 0 else self.score[g0:g0 + n]
                keys.append((base[None, :] - edges[j][:, :n].astype(np.float64)).reshape(-1))
                rows.append(np.tile(np.arange(g0, g0 + n), hi - lo))
                words.append(np.repeat(self.ids[lo:hi].astype(np.int64), n))
                j += 1
            keys, rows, words = np.concatenate(keys), np.concatenate(rows), np.concatenate(words)
            order = np.argsort(keys, kind="stable")
            order = order[~np.isnan(keys[order])][:n_out]
            out.append((keys[order], rows[order], words[order], len(keys)))
        return out

    def run(self, L, n_out, chunk=64, mode=0, stride=None):
        stride = stride or self.F + 1
        R = self.B * n_out
        o = dict(score=torch.full((R + GUARD,), F_FILL, dtype=torch.float64, device="cuda"),
                 row=torch.full((R + GUARD,), I_FILL, dtype=torch.int32, device="cuda"),
                 word=torch.full((R + GUARD,), I_FILL, dtype=torch.int32, device="cuda"),
                 len=torch.full((R + GUARD,), I_FILL, dtype=torch.int32, device="cuda"),
                 nodes=torch.full(((R + GUARD) * stride,), I_FILL, dtype=torch.int32, device="cuda"))
        d = self.d
        rc = L.jlm_tail_predict(self.segs, self.n_segs, d["b2"].data_ptr(), d["T"].data_ptr(), self.ldt, self.B, self.beam, self.F,
                                d["score"].data_ptr(), d["lse"].data_ptr(), d["cnt"].data_ptr(), d["bp"].data_ptr(), d["node"].data_ptr(),
                                mode, d["ids"].data_ptr(), V, d["sp_off"].data_ptr(), d["sp_frame"].data_ptr(), d["sp_lo"].data_ptr(),
                                d["sp_hi"].data_ptr(), n_out, chunk, o["score"].data_ptr(), o["row"].data_ptr(), o["word"].data_ptr(),
                                o["nodes"].data_ptr(), o["len"].data_ptr(), stride, _st())
        assert rc == 0, rc
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in o.items()}
        got["nodes"] = got["nodes"].reshape(R + GUARD, stride)
        for k, fill in (("score", F_FILL), ("row", I_FILL), ("word", I_FILL), ("len", I_FILL), ("nodes", I_FILL)):
            assert (got[k][R:] == fill).all(), "wrote past the outputs: " + k
        return got

    def check(self, L, n_out, chunk=64, mode=0):
        want = self.expected(L, n_out, mode)
        got = self.run(L, n_out, chunk, mode)
        stride = self.F + 1
        for s, (ws, wr, ww, _count) in enumerate(want):
            o, n = s * n_out, len(ws)
            assert got["score"][o:o + n].tobytes() == ws.tobytes(), (s, got["score"][o:o + n], ws)        # bit-equal
            assert got["row"][o:o + n].tolist() == wr.tolist() and got["word"][o:o + n].tolist() == ww.tolist(), s
            assert np.isposinf(got["score"][o + n:o + n_out]).all() and (got["row"][o + n:o + n_out] == -1).all()
            assert (got["word"][o + n:o + n_out] == -1).all() and (got["len"][o + n:o + n_out] == 0).all()
            for r in range(n):
                g, trace = int(wr[r]), []
                while g >= 0 and len(trace) < stride:
                    trace.append(int(self.node[g]))
                    g = int(self.bp[g])
                assert got["len"][o + r] == len(trace) and got["nodes"][o + r, :len(trace)].tolist() == trace, (s, r)
        return want, got


def standard_spans(beam, n_out, rng):
    """a sentence without spans | a span of one word | three spans (one at frame 0) | fewer candidates than n_out (where n_out > 1)"""
    lo = [int(x) for x in rng.integers(0, V - 200, 8)]
    few = max(1, n_out // 2)                       # frame 0 has one hypothesis: one candidate per word
    return [[], [(2, lo[0], lo[0] + 1)], [(0, lo[1], lo[1] + 70), (1, lo[2], lo[2] + 33), (3, lo[3], lo[3] + 97)],
            [(0, lo[4], lo[4] + few)], [(4, lo[5], lo[5] + 45)]]


@pytest.mark.parametrize("n_out", [1, 10, 64])
@pytest.mark.parametrize("beam", [1, 3, 17, 65])
def test_beams_and_list_lengths(L, beam, n_out):
    rng = np.random.default_rng(beam * 100 + n_out)
    p = Problem(MODELS["k32+20"], beam, standard_spans(beam, n_out, rng), seed=beam + n_out)
    p.upload()
    want, _got = p.check(L, n_out)
    assert want[0][3] == 0 and len(want[0][0]) == 0                                   # no spans: padding only
    assert want[1][3] == min(int(p.cnt[2 * p.B + 1]), beam)                           # one word: one candidate per live slot
    assert want[2][3] == 70 + 33 * p.cnt[1 * p.B + 2] + 97 * p.cnt[3 * p.B + 2]
    if n_out > 1:
        assert 0 < want[3][3] < n_out                                                 # fewer candidates than ranks: padded


@pytest.mark.parametrize("name", ["k32", "k512", "k200+100"])
@pytest.mark.parametrize("beam,n_out", [(17, 10), (65, 64)])
def test_models(L, name, beam, n_out):
    rng = np.random.default_rng(7)
    p = Problem(MODELS[name], beam, standard_spans(beam, n_out, rng), seed=11)
    p.upload()
    if len(MODELS[name]) > 1:                                                          # a span's words in both segments
        for f, lo, hi in p.spans[2]:
            assert {bool(w >= V // 2) for w in p.ids[lo:hi]} == {False, True}
    p.check(L, n_out)


def test_chunk_boundaries_and_invariance(L):
    """chunk = the candidate count, one less, 64, and the default; more than 10 000 candidates in one sentence under the default"""
    beam = 17
    p = Problem(MODELS["k32+20"], beam, [[(1, 100, 160), (3, 400, 431)], [(2, 0, 700), (4, 700, 1100)]], seed=3)
    p.cnt[2 * p.B + 1] = p.cnt[4 * p.B + 1] = 16                                     # 17 600 candidates in sentence 1
    p.cnt[1 * p.B + 0], p.cnt[3 * p.B + 0] = 5, 17                                   # (17 rows: a second 16-row pass)
    p.upload()
    count0 = 60 * 5 + 31 * 17
    want = p.expected(L, 10)
    assert want[0][3] == count0 and want[1][3] == 1100 * 16 > 10000
    ref = p.check(L, 10, chunk=0)[1]
    for chunk in (64, count0, count0 - 1, count0 + 1, 513, 4096):
        got = p.check(L, 10, chunk=chunk)[1]
        for k in ref:
            assert got[k].tobytes() == ref[k].tobytes(), (chunk, k)
    ref64 = p.check(L, 64, chunk=0)[1]
    got64 = p.check(L, 64, chunk=64)[1]
    for k in ref64:
        assert got64[k].tobytes() == ref64[k].tobytes(), k


def test_ties_keep_the_lower_slot(L):
    beam = 5
    p = Problem(MODELS["k32"], beam, [[(2, 10, 60)]], seed=5)
    p.cnt[2] = 5
    g0 = 2 * p.rmax
    p.T[g0 + 3] = p.T[g0 + 1]
    p.score[g0 + 3], p.lse[g0 + 3] = p.score[g0 + 1], p.lse[g0 + 1]
    p.score[g0 + 1] -= 50.0                                                            # the tied pair leads the list
    p.score[g0 + 3] -= 50.0
    p.upload()
    want, got = p.check(L, 10)
    rows, words, scores = got["row"][:10], got["word"][:10], got["score"][:10]
    assert set(rows.tolist()) == {g0 + 1, g0 + 3}
    for i in range(0, 10, 2):
        assert scores[i] == scores[i + 1] and words[i] == words[i + 1] and (rows[i], rows[i + 1]) == (g0 + 1, g0 + 3)


def test_nan_lse_never_ranks(L):
    beam = 5
    p = Problem(MODELS["k32+20"], beam, [[(2, 10, 60), (1, 300, 320)]], seed=6)
    p.cnt[2], p.cnt[1] = 4, 3
    p.score[2 * p.rmax + 2] = 0.0
    p.upload()
    clean = p.check(L, 64)[0][0]
    bad = 2 * p.rmax + 2
    assert bad in clean[1]
    p.lse[bad] = np.nan
    p.upload()
    want = p.check(L, 64)[0][0]
    assert bad not in want[1] and not np.isnan(want[0]).any()
    keep = clean[1] != bad                                                             # nothing else moves
    n = min(int(keep.sum()), len(want[0]))
    assert want[1][:n].tolist() == clean[1][keep][:n].tolist() and want[0][:n].tobytes() == clean[0][keep][:n].tobytes()


def test_mode_1_ignores_the_normaliser(L):
    p = Problem(MODELS["k200+100"], 3, standard_spans(3, 10, np.random.default_rng(1)), seed=8)
    p.lse[:] = np.nan                                                                  # a self-normalised model has none
    p.upload()
    want, _got = p.check(L, 10, mode=1)
    assert len(want[2][0]) == 10


def test_refused_arguments(L):
    p = Problem(MODELS["k32"], 3, [[(1, 0, 5)]], seed=9)
    p.upload()
    d = p.d
    o = [torch.zeros(64 * 8, dtype=torch.float64, device="cuda")] + [torch.zeros(64 * 8, dtype=torch.int32, device="cuda") for _ in range(4)]

    def call(n_out=10, beam=3, ldt=p.ldt, lse=d["lse"].data_ptr(), chunk=0, ids=d["ids"].data_ptr(), mode=0, n_sent=1):
        return L.jlm_tail_predict(p.segs, p.n_segs, d["b2"].data_ptr(), d["T"].data_ptr(), ldt, n_sent, beam, p.F, d["score"].data_ptr(), lse,
                                  d["cnt"].data_ptr(), d["bp"].data_ptr(), d["node"].data_ptr(), mode, ids, V, d["sp_off"].data_ptr(),
                                  d["sp_frame"].data_ptr(), d["sp_lo"].data_ptr(), d["sp_hi"].data_ptr(), n_out, chunk, o[0].data_ptr(),
                                  o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(), o[4].data_ptr(), p.F + 1, _st())
    assert call() == 0
    assert call(n_out=0) == -1 and call(n_out=65) == -1
    assert call(beam=1025) == -1 and call(beam=0) == -1
    assert call(ldt=p.ldt + 2) == -1
    assert call(lse=None) == -1 and call(ids=None) == -1
    assert call(lse=None, mode=1) == 0
    assert call(chunk=-1) == -1 and call(chunk=1 << 20) == -1                          # a chunk whose LDS does not fit
    assert call(mode=2) == -1
    assert call(n_sent=0) == 0
    torch.cuda.synchronize()
