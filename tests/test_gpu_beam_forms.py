"""GPU: the beam step and the n-best backtrace in every form the launchers pick, at the boundaries of each form.

Forms (ABI 12: jlm_beam_step_form / jlm_backtrace_form; every launch asserts the library's answer against the numpy restatement in
tests/fake_hip.py, and the backtrace cases against the form each is meant for):

* beam_step_kernel<mode> (one piece): a lane's first 8 candidates in registers, filled by two unrolled groups of 4 x 64, the rest in LDS;
* beam_step_chunked_kernel<mode>: the cell chunk by chunk, then a selection over the chunk winners -- beam 1 024 with 12 nodes per cell
  here, and every case of this module in the children of test_gpu_kernels.py::test_beam_step_chunked_on_ordinary_cells
  (JLM_BEAM_CHUNK = 48, 64, 256), where a case whose chunk winners do not fit LDS must be refused by the form query and is skipped;
* backtrace_wave_kernel<4 | 8 | 16> for beam <= 64 and frames x beam <= 256 / 512 / 1 024, backtrace_kernel (a thread per path) for the
  rest -- and for every case in the child of test_gpu_kernels.py::test_backtrace_thread_per_path_forced (JLM_BACKTRACE_WAVE=0).

The reference is FakeLib.jlm_beam_step / jlm_backtrace: a Python stable sort on (key, candidate index) in float64.  Every input of the
selection tests is dyadic -- lse a multiple of 1/8 in [5, 9], edge logits multiples of 1/2, fused slices in the exact-fold construction
of test_gpu_kernels.py::_run_beam_fused -- so every key is exact in float64 and score / ysum / out_score are compared with ==.  bp, node,
word, cnt, n_live, out_len and out_nodes are compared exactly; live is a set per frame, and live_base -- the position the sentence's
atomicAdd drew, which depends on the order the waves arrive in -- is held to what it promises: live[frame][live_base + r] is the
sentence's row r, and the sentences' ranges tile [0, n_live).

Lattices have prescribed node counts per cell (cells()): frame 0 the root; frame 1 nodes starting at 0, so only slot 0 is valid (a
sparsely valid cell that leaves cnt = min(beam, nodes)); later frames nodes starting at the frame before, the last frame mixing start
frames.  Every cell at frame <= length has a node (include/jlm_hip.h jlm_beam_step: empty cells are not a case).

test_forms_covered needs no GPU: over the parameter lists below it asserts, through the pure form functions of tests/fake_hip.py, that
one-piece, chunked, wave-4, wave-8, wave-16 and thread-per-path each occur."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
from jlm_amd import _lib                                                                                    # noqa: E402
from tests.fake_hip import (BACKTRACE_FORM, BACKTRACE_FORMS, BEAM_STEP_FORM, FakeLib, _atoi_env, backtrace_form,   # noqa: E402
                            beam_step_form)

gpu = pytest.mark.gpu
FK = FakeLib()
CHUNK_ENV = _atoi_env("JLM_BEAM_CHUNK", 0)
WAVE_ENV = _atoi_env("JLM_BACKTRACE_WAVE", 1)
I32_MAX, I32_MIN = np.int32(2 ** 31 - 1), np.int32(-2 ** 31)
MODES = [0, 1, 2]
# largest |device - float64| of the fused fold over FOLD_PARTS measured on the MI355X (profiles/beam_forms_gpu_tests.log); the test holds
# the kernel to 4 x that (the f32 expf rounding varies with the inputs), never above 1e-5 -- half the decode's own score bar (atol 2e-5)
FOLD_MEASURED = 1.185e-7
FOLD_CAP = 1.0e-5


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return _lib.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------ lattices with prescribed cells
def cells(counts, mix_last=True):
    """one sentence: counts[f - 1] nodes in the cell of frame f = 1 .. len -> a list per frame of the nodes' start frames"""
    out = []
    n = len(counts)
    for f in range(1, n + 1):
        if f == 1:
            out.append([0] * counts[0])
        elif f == n and mix_last:
            out.append([max(1, f - 1 - (j % 4 == 3) - (j % 8 == 7)) for j in range(counts[f - 1])])     # most at f - 1, some at f - 2, f - 3
        else:
            out.append([f - 1] * counts[f - 1])
    return out


def lattice(beam, sents, F=None):
    """sents[s] = cells(...) of sentence s -> the CSR arrays of include/jlm_hip.h jlm_lattice (cells ordered by frame, then sentence)"""
    B = len(sents)
    slen = np.array([len(x) for x in sents], np.int32)
    F = F or int(slen.max()) + 1
    counts = np.zeros(F * B, np.int64)
    starts = []
    for f in range(F):
        for s in range(B):
            st = [-1] if f == 0 else (sents[s][f - 1] if f <= slen[s] else [])
            assert f > slen[s] or len(st) >= 1
            counts[f * B + s] = len(st)
            starts += list(st)
    end_off = np.zeros(F * B + 1, np.int32)
    end_off[1:] = np.cumsum(counts)
    N = int(end_off[-1])
    return dict(B=B, beam=beam, F=F, rmax=B * beam, G=F * B * beam, N=N, slen=slen, end_off=end_off,
                nstart=np.array(starts, np.int32), nword=((np.arange(N) * 7 + 3) % 1000).astype(np.int32),
                max_cands=int(counts[B:].max(initial=1)) * beam)


def nb_of(P, f, s):
    return int(P["end_off"][f * P["B"] + s])


def dyadic_inputs(P, seed):
    """lse: multiples of 1/8 in [5, 9]; edge logits: multiples of 1/2 in [-2, 2]"""
    rng = np.random.default_rng(seed)
    lse = rng.integers(40, 73, size=P["G"]).astype(np.float64) / 8.0
    edge = (rng.integers(-4, 5, size=max(P["N"], 1) * P["beam"]) / 2.0).astype(np.float32)
    return lse, edge


def plant(P, edge, f, s, c, value):
    """edge logit of candidate c of cell (f, s)"""
    beam = P["beam"]
    edge[(nb_of(P, f, s) + c // beam) * beam + c % beam] = value


class State:
    """the buffers of jlm_lattice / jlm_beam_state on the GPU (cuda) or in host memory (the reference reads them through the same pointers)"""

    def __init__(self, P, lse, edge, cuda, fill=False, flags=True, n_edge=None):
        self.dev = "cuda" if cuda else "cpu"
        self.cuda, self.P = cuda, P
        G, F, B = P["G"], P["F"], P["B"]
        t = self.t
        self.score = t(np.full(G, np.nan) if fill else np.zeros(G))
        self.ysum = t(np.zeros(G))
        self.lse = t(lse)
        e = np.zeros(max(n_edge or 0, len(edge)), np.float32)
        e[:len(edge)] = edge
        self.edge = t(e)
        ext = np.where(np.arange(G) % 2 == 0, I32_MAX, I32_MIN).astype(np.int32)
        self.bp, self.node, self.word = (t(ext.copy() if fill else np.full(G, -7, np.int32)) for _ in range(3))
        self.cnt, self.live, self.n_live = t(np.zeros(F * B, np.int32)), t(np.full(G, -1, np.int32)), t(np.zeros(F, np.int32))
        self.live_base = t(np.full(F * B, -1, np.int32))
        self.flags = t(np.zeros(1, np.int32)) if flags else None
        self.set_lattice(P)

    def t(self, a):
        return torch.as_tensor(np.array(a, order="C", copy=True)).to(self.dev)      # (a copy: two host states never share an input)

    def set_lattice(self, P):
        self.P = P
        self.ints = {k: self.t(P[k]) for k in ("slen", "end_off", "nstart", "nword")}
        i = self.ints
        self.lat = _lib.Lattice(P["B"], P["beam"], P["F"], i["slen"].data_ptr(), i["end_off"].data_ptr(), i["nstart"].data_ptr(),
                                i["nword"].data_ptr())
        self.st = _lib.BeamState(self.score.data_ptr(), self.lse.data_ptr(), self.ysum.data_ptr(), self.bp.data_ptr(), self.node.data_ptr(),
                                 self.word.data_ptr(), self.cnt.data_ptr(), self.live.data_ptr(), self.n_live.data_ptr(),
                                 self.edge.data_ptr(), self.live_base.data_ptr(), None, 0, 0,
                                 self.flags.data_ptr() if self.flags is not None else None)

    def sync(self):
        if self.cuda:
            torch.cuda.synchronize()

    def out(self):
        self.sync()
        names = ("score", "ysum", "lse", "bp", "node", "word", "cnt", "live", "n_live", "live_base")
        d = {k: getattr(self, k).cpu().numpy().copy() for k in names}
        d["flags"] = int(self.flags.cpu().numpy()[0]) if self.flags is not None else None
        return d


def step_form(L, P, mode, max_cands):
    """the library's form for this launch, pinned to the numpy restatement; under JLM_BEAM_CHUNK every launch is chunked, and a case whose
    chunk winners do not fit LDS is refused before any launch: skipped, not run"""
    got = L.jlm_beam_step_form(P["beam"], P["F"], mode, max_cands)
    assert got == FK.jlm_beam_step_form(P["beam"], P["F"], mode, max_cands) == beam_step_form(P["beam"], P["F"], mode, max_cands, CHUNK_ENV)
    if got < 0:
        assert CHUNK_ENV > 0, "refused without JLM_BEAM_CHUNK"
        pytest.skip("JLM_BEAM_CHUNK=%d: the chunk winners of %d candidates at beam %d do not fit LDS" % (CHUNK_ENV, max_cands, P["beam"]))
    if CHUNK_ENV > 0:
        assert got == BEAM_STEP_FORM["CHUNKED"]
    return got


def run_steps(lib, S, mode, max_cands, frames=None):
    P = S.P
    for f in (range(P["F"]) if frames is None else frames):
        assert lib.jlm_beam_step(S.lat, S.st, f, mode, max_cands, _stream() if S.cuda else 0) == 0


def run_backtrace(lib, S, stride):
    P = S.P
    rmax = P["rmax"]
    on, ol, osc = S.t(np.full((rmax + 2) * stride, -1, np.int32)), S.t(np.full(rmax + 2, -9, np.int32)), S.t(np.full(rmax + 2, 7.0))
    assert lib.jlm_backtrace(S.lat, S.st, on.data_ptr(), ol.data_ptr(), osc.data_ptr(), stride, _stream() if S.cuda else 0) == 0
    S.sync()
    return on.cpu().numpy(), ol.cpu().numpy(), osc.cpu().numpy()


def bt_form(L, P, expect=None):
    got = L.jlm_backtrace_form(P["beam"], P["F"])
    assert got == FK.jlm_backtrace_form(P["beam"], P["F"]) == backtrace_form(P["beam"], P["F"], WAVE_ENV)
    if WAVE_ENV == 0:
        assert got == BACKTRACE_FORM["THREAD"]
    elif expect is not None:
        assert got == BACKTRACE_FORM[expect], (BACKTRACE_FORMS[got], expect)
    return got


def check_backtrace(L, Sg, Sc, stride, expect=None):
    bt_form(L, Sg.P, expect)
    got, want = run_backtrace(L, Sg, stride), run_backtrace(FK, Sc, stride)
    np.testing.assert_array_equal(got[1], want[1])                       # out_len (rows at and above the final cnt: 0)
    assert np.array_equal(got[2], want[2]), np.abs(got[2] - want[2]).max()   # out_score, ==
    np.testing.assert_array_equal(got[0], want[0])                       # out_nodes: the paths, and -1 wherever no path was written
    return want


def check_state(got, want, P, mode, frames=None):
    B, beam, rmax = P["B"], P["beam"], P["rmax"]
    np.testing.assert_array_equal(got["cnt"], want["cnt"])
    np.testing.assert_array_equal(got["n_live"], want["n_live"])
    for f in (range(P["F"]) if frames is None else frames):
        spans = []
        for s in range(B):
            k = int(want["cnt"][f * B + s])
            g0 = f * rmax + s * beam
            sl = slice(g0, g0 + k)
            for name in ("bp", "node", "word"):
                np.testing.assert_array_equal(got[name][sl], want[name][sl], err_msg="%s f=%d s=%d" % (name, f, s))
            assert np.array_equal(got["score"][sl], want["score"][sl]), ("score", f, s, got["score"][sl], want["score"][sl])
            if mode == 2:
                assert np.array_equal(got["ysum"][sl], want["ysum"][sl]), ("ysum", f, s)
            if f < int(P["slen"][s]) and k:
                base = int(got["live_base"][f * B + s])
                np.testing.assert_array_equal(got["live"][f * rmax + base:f * rmax + base + k], np.arange(g0, g0 + k), err_msg="live_base f=%d s=%d" % (f, s))
                spans.append((base, k))
        nl = int(want["n_live"][f])
        assert sorted(got["live"][f * rmax:f * rmax + nl]) == sorted(want["live"][f * rmax:f * rmax + nl])
        pos = 0
        for base, k in sorted(spans):
            assert base == pos, ("live_base ranges do not tile the frame's list", f, spans)
            pos += k
        assert pos == nl


def compare(L, P, mode, lse, edge, max_cands=None, backtrace=False, expect=None):
    """all frames on the device and in the reference, compared row by row; -> (form, the reference's state)"""
    mc = P["max_cands"] if max_cands is None else max_cands
    form = step_form(L, P, mode, mc)
    if expect is not None and CHUNK_ENV <= 0:
        assert form == BEAM_STEP_FORM[expect]
    Sc, Sg = State(P, lse, edge, False), State(P, lse, edge, True)
    run_steps(FK, Sc, mode, mc)
    run_steps(L, Sg, mode, mc)
    want, got = Sc.out(), Sg.out()
    check_state(got, want, P, mode)
    if backtrace:
        check_backtrace(L, Sg, Sc, P["F"] + 1)
    return form, want


# ------------------------------------------------------------------ every index wins
def index_problem():
    """B = 64, beam 20, one cell of 55 nodes (C = 1 100 = 17 x 64 + 12): sentence s plants its 20 largest edge logits, distinct and well
    above the rest (keys of the rest differ by less than 20), at candidates (20 s + j) mod C"""
    B, beam, n = 64, 20, 55
    P = lattice(beam, [cells([beam, n], mix_last=False) for _ in range(B)])
    lse, edge = dyadic_inputs(P, 1100)
    C = n * beam
    for s in range(B):
        for j in range(beam):
            plant(P, edge, 2, s, (beam * s + j) % C, 100.0 + 0.5 * j)
    return P, lse, edge, C


@gpu
@pytest.mark.parametrize("rounded", [0, 1], ids=["exact", "rounded256"])
@pytest.mark.parametrize("mode", MODES)
def test_every_index_wins(L, mode, rounded):
    """every register slot and LDS entry of the one-piece kernel holds a winner once: the union over the sentences of the candidate
    indices that won -- computed from the reference's output -- is all of 0 .. C - 1; with max_cands exact and rounded up to a multiple of
    256 (as the decode passes it: every LDS array behind keys[] moves)"""
    P, lse, edge, C = index_problem()
    mc = P["max_cands"] if not rounded else (P["max_cands"] + 255) // 256 * 256
    assert (mc == 1100) != bool(rounded) and mc >= C
    _, want = compare(L, P, mode, lse, edge, mc, expect="ONE_PIECE")
    won = set()
    B, beam, rmax = P["B"], P["beam"], P["rmax"]
    for s in range(B):
        assert want["cnt"][2 * B + s] == beam
        for r in range(beam):
            g = 2 * rmax + s * beam + r
            won.add((int(want["node"][g]) - nb_of(P, 2, s)) * beam + int(want["bp"][g]) - (rmax + s * beam))
    assert won == set(range(C)), sorted(set(range(C)) - won)[:8]


# ------------------------------------------------------------------ boundaries of C
BOUNDARY_C = {1: (1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 768, 769), 3: (3, 63, 66, 255, 258, 510, 513, 768, 771)}
PLANT_AT = (0, "last", 63, 64, 255, 256, 511, 512)         # the ends of a lane's row, of the two register groups (4 x 64 each), of the cell


def boundary_problem(beam):
    """frame f = 2 .. holds a cell of C = BOUNDARY_C[beam][f - 2] candidates; sentence s plants the winner of every cell at PLANT_AT[s]
    (where the cell is that long), at least 60 above the rest and 32 above the plant of the frame before"""
    counts = [max(beam, 2)] + [c // beam for c in BOUNDARY_C[beam]]
    P = lattice(beam, [cells(counts, mix_last=False) for _ in PLANT_AT])
    lse, edge = dyadic_inputs(P, 7 + beam)
    for s, at in enumerate(PLANT_AT):
        for i, C in enumerate(BOUNDARY_C[beam]):
            c = C - 1 if at == "last" else at
            if c < C:
                plant(P, edge, 2 + i, s, c, 64.0 + 32.0 * i)    # (rank 0 of the frame before is ahead by about its plant: 32 more wins from any slot)
    return P, lse, edge


@gpu
@pytest.mark.parametrize("beam", [1, 3])
@pytest.mark.parametrize("mode", MODES)
def test_boundaries_of_c(L, mode, beam):
    """C = 1, 63, 64, 65 (one candidate per lane, one more), 255 .. 257 and 511 .. 513 (the ends of the two register groups), 768, 769 and
    C no multiple of 64 (beam 3: the nearest multiples of 3), the winner at index 0, at C - 1 and at the last index of each group"""
    P, lse, edge = boundary_problem(beam)
    _, want = compare(L, P, mode, lse, edge, backtrace=True)
    B, rmax = P["B"], P["rmax"]
    for s, at in enumerate(PLANT_AT):                          # (the construction: the planted candidate is the reference's rank 0)
        for i, C in enumerate(BOUNDARY_C[beam]):
            c = C - 1 if at == "last" else at
            if c < C:
                g = (2 + i) * rmax + s * beam
                assert int(want["node"][g]) - nb_of(P, 2 + i, s) == c // beam and int(want["bp"][g]) == (1 + i) * rmax + s * beam + c % beam


# ------------------------------------------------------------------ ties
TIE_BEAM, TIE_NODES = 3, 260                                   # C = 780 = 12 x 64 + 12
TIE_GROUPS = [[62, 63, 64, 65, 66], [254, 255, 256, 257, 258], [510, 511, 512, 513, 514],
              [5 + 64 * j for j in (6, 7, 8, 9, 10)],          # one lane's slots 6 .. 10: across the register / LDS line (slots 7 and 8)
              [63 + 64 * 7, 64 * 8, 63 + 64 * 8, 64 * 9, 700],
              list(range(TIE_BEAM * TIE_NODES))] + \
             [[cap - 1, cap, 2 * cap, 2 * cap + 1, 3 * cap] for cap in (48, 64, 256)]   # the chunked children's chunk boundaries


def tie_problem(mode):
    """beam 3: frame 1 leaves rows k = 0, 1, 2 with scores 0.5 k apart, and in modes 0 and 2 their lse = 8.125 - 0.5 k makes score + lse
    the same for every predecessor: there the ties come from lse (equal edge logits), in mode 1 from edge logits 0.5 k apart.  Sentence
    s ties the beam + 2 (or all) candidates TIE_GROUPS[s] of the frame-2 cell at the best key, 15 below every other"""
    beam = TIE_BEAM
    P = lattice(beam, [cells([4, TIE_NODES], mix_last=False) for _ in TIE_GROUPS])
    lse, edge = dyadic_inputs(P, 33)
    rmax = P["rmax"]
    for s, grp in enumerate(TIE_GROUPS):
        nb1 = nb_of(P, 1, s)
        for j in range(4):
            edge[(nb1 + j) * beam] = -0.5 * j if j < 3 else -10.0
        for k in range(beam):
            lse[rmax + s * beam + k] = 8.125 - 0.5 * k
        for c in grp:
            plant(P, edge, 2, s, c, 20.0 + (0.5 * (c % beam) if mode == 1 else 0.0))
    return P, lse, edge


@gpu
@pytest.mark.parametrize("mode", MODES)
def test_ties(L, mode):
    """more candidates tied at the best key than free ranks -- across lanes (63 | 64), across the register groups (255 | 256, 511 | 512),
    across one lane's register / LDS line, across chunk boundaries (cap - 1 | cap | 2 cap) and a whole cell: the survivors are the lowest
    candidate indices, in index order"""
    P, lse, edge = tie_problem(mode)
    _, want = compare(L, P, mode, lse, edge)
    beam, rmax = P["beam"], P["rmax"]
    for s, grp in enumerate(TIE_GROUPS):
        g = 2 * rmax + s * beam
        assert len(grp) >= beam + 2 and want["cnt"][2 * P["B"] + s] == beam
        won = [(int(want["node"][g + r]) - nb_of(P, 2, s)) * beam + int(want["bp"][g + r]) - (rmax + s * beam) for r in range(beam)]
        assert won == sorted(grp)[:beam], (s, won)
        assert len(set(want["score"][g:g + beam])) == 1


# ------------------------------------------------------------------ wide beams, long sentences
WIDE = [(65, 3, 6, 12), (100, 3, 6, 12), (257, 3, 6, 12), (1024, 2, 4, 11), (1024, 2, 4, 12)]


def wide_problem(beam, B, F, nodes):
    """`nodes` per cell: cnt grows 12, 144, ... up to the beam, so counts below the beam and equal to it both occur; the sentences end at
    different frames"""
    sents = [cells([nodes] * max(F - 1 - s, 1)) for s in range(B)]
    P = lattice(beam, sents, F)
    return (P,) + dyadic_inputs(P, beam + nodes)


@gpu
@pytest.mark.parametrize("beam,B,F,nodes", WIDE)
@pytest.mark.parametrize("mode", MODES)
def test_wide_beams(L, mode, beam, B, F, nodes):
    """beams above one wave (a lane writes ranks lane, lane + 64, ...) up to JLM_MAX_BEAM, row by row; beam 1 024 with 12 nodes per cell
    (12 288 candidates) is past one wave's LDS: the chunked kernel without any setting"""
    P, lse, edge = wide_problem(beam, B, F, nodes)
    form, want = compare(L, P, mode, lse, edge, backtrace=True)
    if CHUNK_ENV <= 0:
        assert form == beam_step_form(beam, F, mode, P["max_cands"], 0)
        if beam == 1024 and nodes == 12:
            assert form == BEAM_STEP_FORM["CHUNKED"]
    live_cnt = [int(want["cnt"][f * B + s]) for s in range(B) for f in range(1, int(P["slen"][s]) + 1)]
    assert min(live_cnt) < beam and max(live_cnt) == beam


LONG_F = [70, 130]


def long_problem(F):
    """B = 2, beam 3: one sentence of full length, one of length 1 (its rows of every later frame: cnt = 0)"""
    counts = [3] + [2 + f % 3 for f in range(2, F)]
    full = [[0] * 3] + [[max(1, f - 1 - (j % 4)) for j in range(counts[f - 1])] for f in range(2, F)]
    P = lattice(3, [full, cells([4])], F)
    return (P,) + dyadic_inputs(P, F)


@gpu
@pytest.mark.parametrize("F", LONG_F)
@pytest.mark.parametrize("mode", MODES)
def test_long_sentences(L, mode, F):
    """more than 64 frames (the load of the sentence's counts strides by 64; 130: a third pass), and the frame > length rows"""
    P, lse, edge = long_problem(F)
    _, want = compare(L, P, mode, lse, edge, backtrace=True)
    assert (want["cnt"][2 * P["B"] + 1::P["B"]] == 0).all() and (want["cnt"][0::P["B"]] > 0).all()


# ------------------------------------------------------------------ reused state
def reuse_problems():
    B, beam, F = 4, 5, 7
    P1 = lattice(beam, [cells([7, 9, 13, 4, 6, 8]), cells([5, 3, 2]), cells([6, 14, 3, 3, 9]), cells([9])], F)
    P2 = lattice(beam, [cells([6, 2]), cells([5, 11, 7, 2, 3, 5]), cells([8]), cells([5, 4, 13, 6])], F)
    return P1, P2


@gpu
@pytest.mark.parametrize("mode", MODES)
def test_reused_state(L, mode):
    """two different problems back to back on the same device buffers, as a decode plan serves its batches: between them only cnt,
    n_live and the flag word are zeroed (jlm_amd/engine.py), max_cands is rounded up to a multiple of 256, and before the first run bp /
    node / word / score hold INT32 extremes and NaN.  The second result is the reference's on fresh buffers; the backtrace follows on the
    same state"""
    P1, P2 = reuse_problems()
    mc = (max(P1["max_cands"], P2["max_cands"]) + 255) // 256 * 256
    step_form(L, P1, mode, mc)
    in1, in2 = dyadic_inputs(P1, 51), dyadic_inputs(P2, 52)
    n_edge = max(len(in1[1]), len(in2[1]))
    Sg = State(P1, in1[0], in1[1], True, fill=True, n_edge=n_edge)
    run_steps(L, Sg, mode, mc)
    first = Sg.out()
    Sc1 = State(P1, in1[0], in1[1], False)
    run_steps(FK, Sc1, mode, mc)
    check_state(first, Sc1.out(), P1, mode)
    Sg.cnt.zero_(); Sg.n_live.zero_(); Sg.flags.zero_()
    Sg.lse.copy_(Sg.t(in2[0]))
    Sg.edge[:len(in2[1])].copy_(Sg.t(in2[1]))
    Sg.set_lattice(P2)
    run_steps(L, Sg, mode, mc)
    Sc = State(P2, in2[0], in2[1], False)
    run_steps(FK, Sc, mode, mc)
    check_state(Sg.out(), Sc.out(), P2, mode)
    check_backtrace(L, Sg, Sc, P2["F"] + 1)


# ------------------------------------------------------------------ backtrace forms
BT_CASES = [(64, 4, "WAVE4"), (3, 86, "WAVE8"), (64, 8, "WAVE8"), (57, 9, "WAVE16"), (64, 16, "WAVE16"), (41, 25, "THREAD"),
            (65, 3, "THREAD")]          # frames x beam = 256, 258, 512, 513, 1 024, 1 025; beam 65


def backtrace_state(beam, F, cuda):
    """a beam state written directly (the backtrace reads sent_len, cnt, score, bp and node only): three sentences -- full length, half,
    and 3 -- with counts between 1 and the beam (the final count below the beam in one sentence, equal to it in another), back-pointers to
    a live row one to three frames back, and INT32 extremes in every row at and above a cell's count"""
    B = 3
    rng = np.random.default_rng(beam * 1000 + F)
    lens = [F - 1, max((F - 1) // 2, min(3, F - 1)), min(3, F - 1)]
    P = lattice(beam, [cells([1] * n) for n in lens], F)
    rmax, G = P["rmax"], P["G"]
    S = State(P, np.zeros(G), np.zeros(1, np.float32), cuda, fill=True)
    cnt = np.zeros(F * B, np.int32)
    bp = np.where(np.arange(G) % 2 == 0, I32_MAX, I32_MIN).astype(np.int32)
    node = bp[::-1].copy()
    score = np.full(G, np.nan)
    for s in range(B):
        for f in range(lens[s] + 1):
            c = 1 if f == 0 else int(rng.integers(1, beam + 1))
            if f == lens[s]:
                c = beam if s == 0 else max(beam - 2, 1) if s == 1 else c
            cnt[f * B + s] = c
            for k in range(c):
                g = f * rmax + s * beam + k
                node[g] = int(rng.integers(0, 100000))
                score[g] = float(rng.integers(-4000, 4000)) / 8.0
                if f == 0:
                    bp[g] = -1
                else:
                    pf = int(rng.integers(max(0, f - 3), f))
                    bp[g] = pf * rmax + s * beam + int(rng.integers(0, cnt[pf * B + s]))
    for name, a in (("cnt", cnt), ("bp", bp), ("node", node), ("score", score)):
        getattr(S, name).copy_(S.t(a))
    return S, lens


@gpu
@pytest.mark.parametrize("short", [0, 1], ids=["stride=F+1", "stride=2"])
@pytest.mark.parametrize("beam,F,form", BT_CASES)
def test_backtrace_forms(L, beam, F, form, short):
    """each backtrace kernel at the limits of the shapes it serves; stride F + 1 (whole paths) and stride 2 on sentences longer than 2
    (truncated paths, the reference's lengths); rows at and above a sentence's final count: length 0, score 0"""
    Sg, lens = backtrace_state(beam, F, True)
    Sc, _ = backtrace_state(beam, F, False)
    stride = 2 if short else F + 1
    on, ol, osc = check_backtrace(L, Sg, Sc, stride, form)
    cnt = Sc.cnt.numpy()
    for s in range(3):
        c = int(cnt[lens[s] * 3 + s])
        assert (ol[s * beam:s * beam + c] > 0).all() and (ol[s * beam + c:(s + 1) * beam] == 0).all()
        assert (osc[s * beam + c:(s + 1) * beam] == 0.0).all()
        if short:
            assert (ol[s * beam:s * beam + c] == min(2, lens[s] + 1)).all()
    assert ol.max() <= stride and (not short or lens[0] + 1 > 2)


# ------------------------------------------------------------------ the fused fold of the vocabulary partials
FOLD_PARTS = [1, 5, 7, 8, 9, 24]


def fold_problem():
    """beam 11, previous counts 1, 5 and 11 (none a multiple of the fold's 8 rows per pass)"""
    return lattice(11, [cells([11, 3, 4]), cells([5, 3, 2]), cells([13, 2, 5])])


def run_fused(lib, S, table, max_cands, frames=None):
    """mode 0 with the log-normalisers arriving as n_parts slices of (max, sum exp) indexed by live position: table[q, g] is slice q of
    hypothesis row g, wherever the frame's list holds it"""
    P = S.P
    rmax, n_parts = P["rmax"], table.shape[0]
    part = S.t(np.zeros((n_parts, rmax, 2), np.float32))
    S.keep = part
    for f in (range(P["F"]) if frames is None else frames):
        if f >= 1:
            S.sync()
            nl = int(S.n_live[f - 1].item())
            lv = S.live[(f - 1) * rmax:(f - 1) * rmax + nl].cpu().numpy().astype(np.int64)
            pn = np.zeros((n_parts, rmax, 2), np.float32)
            pn[:, :nl] = table[:, lv]
            part.copy_(S.t(pn))
            S.st.lse_part, S.st.ld_part, S.st.n_parts = part.data_ptr(), rmax, n_parts
        assert lib.jlm_beam_step(S.lat, S.st, f, 0, max_cands, _stream() if S.cuda else 0) == 0
    S.sync()


@gpu
@pytest.mark.parametrize("n_parts", FOLD_PARTS)
def test_fused_fold_numerics(L, n_parts):
    """the fold of n_parts = 1, 5, 7, 8, 9, 24 slices (8 lanes per row: fewer slices than lanes, an odd count, one more than a pass) with
    maxima uniform in [-5, 15] and sums log-uniform in [1, 1e4], lse only, against the float64 fold of the same f32 slices.
    Measured on the MI355X: largest |device - float64| = 1.185e-7 over these cases (n_parts 1: 0, 5: 1.185e-7, 7: 5.04e-8, 8: 9.60e-8,
    9: 8.14e-8, 24: 5.56e-8); asserted at 4 x that (4.74e-7), never above 1e-5."""
    P = fold_problem()
    step_form(L, P, 0, P["max_cands"])
    rng = np.random.default_rng(n_parts)
    G, rmax, beam, B = P["G"], P["rmax"], P["beam"], P["B"]
    table = np.zeros((n_parts, G, 2), np.float32)
    table[:, :, 0] = rng.uniform(-5.0, 15.0, size=(n_parts, G)).astype(np.float32)
    table[:, :, 1] = np.exp(rng.uniform(0.0, np.log(1.0e4), size=(n_parts, G))).astype(np.float32)
    lse0, edge = dyadic_inputs(P, 3)
    S = State(P, np.full(G, 1.0e30), edge, True)
    run_fused(L, S, table, P["max_cands"])
    got = S.out()
    assert got["flags"] == 0
    t64 = table.astype(np.float64)
    worst, n = 0.0, 0
    for f in range(P["F"] - 1):
        for s in range(B):
            if f >= int(P["slen"][s]):
                continue
            k = int(got["cnt"][f * B + s])
            assert k in ((1,) if f == 0 else (5, 11) if f == 1 else range(1, 12))
            for g in range(f * rmax + s * beam, f * rmax + s * beam + k):
                mx = t64[:, g, 0].max()
                want = mx + np.log((t64[:, g, 1] * np.exp(t64[:, g, 0] - mx)).sum())
                worst = max(worst, abs(got["lse"][g] - want))
                n += 1
    print("fused fold n_parts=%d rows=%d max |device - f64| = %.3e" % (n_parts, n, worst))
    assert n >= 17
    tol = min(4.0 * FOLD_MEASURED, FOLD_CAP)
    assert worst <= tol, (worst, tol)


def exact_table(P, n_parts):
    """slices whose fold is exact in any arithmetic: three slices of row g at its maximum 3 + g % 5 with sums 1/2, 1/4, 1/4, starting at
    slice g % n_parts, every other slice 200 below (exp underflows to 0 in f32 and is absorbed in f64): the sum is 1, lse the maximum"""
    assert n_parts >= 3
    g = np.arange(P["G"], dtype=np.int64)
    table = np.zeros((n_parts, P["G"], 2), np.float32)
    for q in range(n_parts):
        j = (q - g) % n_parts
        table[q, :, 0] = 3.0 + (g % 5) - 200.0 * (j >= 3)
        table[q, :, 1] = np.where(j == 0, 0.5, np.where(j < 3, 0.25, 1.0 + (g + 3 * q) % 7))
    return table


@gpu
@pytest.mark.parametrize("with_flags", [1, 0], ids=["flags", "flags=NULL"])
def test_fused_fold_nonfinite(L, with_flags):
    """one row's slices hold +inf, one row's a NaN, one row's sums are all 0: the flag word becomes 1 (where there is one), those rows' lse
    is 1e30 and every other row the reference's; the counts are those of the run without the poison -- the search goes on"""
    P = fold_problem()
    mc = P["max_cands"]
    step_form(L, P, 0, mc)
    n_parts, rmax, beam = 9, P["rmax"], P["beam"]
    clean = exact_table(P, n_parts)
    table = clean.copy()
    rows = [rmax + 0 * beam + 1, rmax + 1 * beam + 0, rmax + 2 * beam + 2]         # frame 1: a row of each sentence
    table[0, rows[0], 0] = np.inf
    table[n_parts - 1, rows[1], 0] = np.nan
    table[:, rows[2], 1] = 0.0
    _, edge = dyadic_inputs(P, 4)
    lse = np.full(P["G"], 1.0e30)
    Sg, Sc, Sclean = State(P, lse, edge, True, flags=bool(with_flags)), State(P, lse, edge, False, flags=bool(with_flags)), State(P, lse, edge, False)
    run_fused(L, Sg, table, mc)
    run_fused(FK, Sc, table, mc)
    run_fused(FK, Sclean, clean, mc)
    got, want, ref = Sg.out(), Sc.out(), Sclean.out()
    assert got["flags"] == want["flags"] == (1 if with_flags else None) and ref["flags"] == 0
    np.testing.assert_array_equal(want["cnt"], ref["cnt"])
    check_state(got, want, P, 0)
    B = P["B"]
    for f in range(P["F"] - 1):
        for s in range(B):
            if f < int(P["slen"][s]):
                k = int(want["cnt"][f * B + s])
                sl = slice(f * rmax + s * beam, f * rmax + s * beam + k)
                assert np.array_equal(got["lse"][sl], want["lse"][sl]), (f, s, got["lse"][sl], want["lse"][sl])
    assert (got["lse"][rows] == 1.0e30).all()
    assert np.isfinite(got["lse"][rmax:rmax + beam]).all() and (np.delete(got["lse"][rmax:rmax + beam], 1) < 1.0e3).all()


# ------------------------------------------------------------------ the forms the parameter lists reach (no GPU)
def step_shapes():
    """(beam, n_frames, mode, max_cands) of every beam-step launch the cases above make"""
    probs = [index_problem()[0], fold_problem()] + [boundary_problem(b)[0] for b in BOUNDARY_C] + [tie_problem(0)[0]]
    probs += [wide_problem(*w)[0] for w in WIDE] + [long_problem(F)[0] for F in LONG_F]
    return [(P["beam"], P["F"], mode, P["max_cands"]) for P in probs for mode in MODES]


def test_forms_covered():
    """every form occurs among the values the cases assert, with no setting in the environment: one piece and chunked for the beam step,
    wave-4 / 8 / 16 and thread per path for the backtrace (each backtrace case names the form it is meant for)"""
    steps = {beam_step_form(*shape, 0) for shape in step_shapes()}
    assert steps == {BEAM_STEP_FORM["ONE_PIECE"], BEAM_STEP_FORM["CHUNKED"]}, steps
    for beam, F, name in BT_CASES:
        assert backtrace_form(beam, F, 1) == BACKTRACE_FORM[name], (beam, F, name)
        assert backtrace_form(beam, F, 0) == BACKTRACE_FORM["THREAD"]
    assert {name for _, _, name in BT_CASES} == set(BACKTRACE_FORMS)
    assert sorted(F * b for b, F, _ in BT_CASES) == [195, 256, 258, 512, 513, 1024, 1025]
    # the forced settings: every case is chunked or refused, never one piece
    for chunk in (48, 64, 256):
        forced = {beam_step_form(*shape, chunk) for shape in step_shapes()}
        assert forced == {BEAM_STEP_FORM["CHUNKED"], -1}, (chunk, forced)
