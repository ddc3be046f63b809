"""GPU: the one-piece beam step after its loads were batched (DESIGN.md 4.1 "chain trips"): the fused fold takes a lane's slices 4 per row
and 2 rows at a time (one batch = 32 slices x 16 rows, a loop over batches beyond), and the candidates' loads go out eight candidates of
a lane at a time.  The arithmetic and its order are the earlier kernel's, so every check here is the one test_gpu_beam_forms.py makes --
whose helpers this module imports -- at the shapes where the new batching changes path:

* fold: n_parts 1, 7, 8, 9 (fewer slices than a row's 8 lanes, one more), 31, 32, 33 (one batch, one more), 64, 99 (MX_MAX_SUB: a fourth,
  partial batch); previous cells of 1, 8, 9, 10 and 16 rows (one row pass, one more row, the beam, two full passes) at beam 10 and 16.
  Slices in the exact-fold construction (equal maxima, dyadic sums: exact in any order) are held to == the float64 value and the whole
  state to the reference's; general slices to 4.74e-7 of the float64 fold, the bar of test_gpu_beam_forms.py::test_fused_fold_numerics
  (DESIGN.md 7); the non-finite branch to its contract (flag word, 1e30, the counts of the clean run);
* candidates: cells of C = 1 .. 1 024 candidates around every multiple of 64 x 4 with dyadic keys, winners and ties planted across the
  ends of a lane's row and of each group of 4 x 64 and 8 x 64; == Python's stable sort (FakeLib), the form asserted in every case;
* a second problem on the same device buffers with only cnt, n_live and the flag word cleared, fused."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
from tests.fake_hip import FakeLib                                                                     # noqa: E402
from tests.test_gpu_beam_forms import (L, State, cells, check_backtrace, check_state, compare, dyadic_inputs,   # noqa: E402,F401
                                       exact_table, lattice, nb_of, plant, run_fused, step_form)

gpu = pytest.mark.gpu
FK = FakeLib()
FOLD_TOL = 4.74e-7                      # 4 x the largest |device - float64| measured for the fold (tests/test_gpu_beam_forms.py)
FOLD_PARTS = [1, 7, 8, 9, 31, 32, 33, 64, 99]
FOLD_ROWS = [1, 8, 9, 10, 16]
BEAMS = [10, 16]


def fold_problem(beam):
    """sentence i: FOLD_ROWS[i] nodes in the cell of frame 1, all starting at frame 0 where only slot 0 is live -> the cell keeps
    min(beam, FOLD_ROWS[i]) rows, which the step of frame 2 folds; the step of frame 1 folds the single row of frame 0"""
    return lattice(beam, [cells([n, 3, 2]) for n in FOLD_ROWS])


def fold_rows(P, got):
    """(row g, frame, sentence) of every row a fused step has folded"""
    B, beam, rmax = P["B"], P["beam"], P["rmax"]
    out = []
    for f in range(P["F"] - 1):
        for s in range(B):
            if f < int(P["slen"][s]):
                k = int(got["cnt"][f * B + s])
                out += [(g, f, s) for g in range(f * rmax + s * beam, f * rmax + s * beam + k)]
    return out


def exact_slices(P, n_parts):
    if n_parts >= 3:
        return exact_table(P, n_parts)
    table = np.zeros((n_parts, P["G"], 2), np.float32)           # one slice: the maximum with sum 1
    table[:, :, 0] = 3.0 + (np.arange(P["G"]) % 5)
    table[:, :, 1] = 1.0
    assert n_parts == 1
    return table


@gpu
@pytest.mark.parametrize("n_parts", FOLD_PARTS)
@pytest.mark.parametrize("beam", BEAMS)
def test_fold_exact(L, beam, n_parts):
    """equal maxima and dyadic sums: lse == the float64 value (the row's maximum), and the whole search == the reference's"""
    P = fold_problem(beam)
    mc = P["max_cands"]
    step_form(L, P, 0, mc)
    table = exact_slices(P, n_parts)
    _, edge = dyadic_inputs(P, 5 + n_parts)
    lse = np.full(P["G"], 1.0e30)
    Sg, Sc = State(P, lse, edge, True), State(P, lse, edge, False)
    run_fused(L, Sg, table, mc)
    run_fused(FK, Sc, table, mc)
    got, want = Sg.out(), Sc.out()
    assert got["flags"] == want["flags"] == 0
    check_state(got, want, P, 0)
    rows = fold_rows(P, want)
    B = P["B"]
    assert sorted({int(want["cnt"][B + s]) for s in range(B)}) == sorted({min(beam, n) for n in FOLD_ROWS})
    for g, f, s in rows:
        assert got["lse"][g] == 3.0 + g % 5 == want["lse"][g], (g, f, s, got["lse"][g])


@gpu
@pytest.mark.parametrize("n_parts", FOLD_PARTS)
@pytest.mark.parametrize("beam", BEAMS)
def test_fold_general(L, beam, n_parts):
    """maxima uniform in [-5, 15], sums log-uniform in [1, 1e4]: every folded row within 4.74e-7 of the float64 fold of the same slices"""
    P = fold_problem(beam)
    mc = P["max_cands"]
    step_form(L, P, 0, mc)
    rng = np.random.default_rng(1000 * beam + n_parts)
    G = P["G"]
    table = np.zeros((n_parts, G, 2), np.float32)
    table[:, :, 0] = rng.uniform(-5.0, 15.0, size=(n_parts, G)).astype(np.float32)
    table[:, :, 1] = np.exp(rng.uniform(0.0, np.log(1.0e4), size=(n_parts, G))).astype(np.float32)
    _, edge = dyadic_inputs(P, 3)
    S = State(P, np.full(G, 1.0e30), edge, True)
    run_fused(L, S, table, mc)
    got = S.out()
    assert got["flags"] == 0
    t64 = table.astype(np.float64)
    rows = fold_rows(P, got)
    assert len(rows) >= len(FOLD_ROWS) + sum(min(beam, n) for n in FOLD_ROWS)
    worst = 0.0
    for g, _f, _s in rows:
        mx = t64[:, g, 0].max()
        worst = max(worst, abs(got["lse"][g] - (mx + np.log((t64[:, g, 1] * np.exp(t64[:, g, 0] - mx)).sum()))))
    print("fold beam=%d n_parts=%d rows=%d max |device - f64| = %.3e" % (beam, n_parts, len(rows), worst))
    assert worst <= FOLD_TOL, (worst, FOLD_TOL)


@gpu
@pytest.mark.parametrize("n_parts", [9, 33, 99])
def test_fold_nonfinite(L, n_parts):
    """beam 16, the 16-row cell: +inf in a slice of a first-pass row, a NaN in the last slice of a second-pass row, all sums 0 in a third
    -- the flag word becomes 1, those rows' lse 1e30, every other row the reference's, and the counts are the clean run's"""
    P = fold_problem(16)
    mc = P["max_cands"]
    step_form(L, P, 0, mc)
    rmax, beam, B = P["rmax"], P["beam"], P["B"]
    s16 = FOLD_ROWS.index(16)
    clean = exact_table(P, n_parts)
    table = clean.copy()
    rows = [rmax + s16 * beam + 3, rmax + s16 * beam + 12, rmax + FOLD_ROWS.index(9) * beam + 8]
    table[n_parts // 2, rows[0], 0] = np.inf
    table[n_parts - 1, rows[1], 0] = np.nan
    table[:, rows[2], 1] = 0.0
    _, edge = dyadic_inputs(P, 4)
    lse = np.full(P["G"], 1.0e30)
    Sg, Sc, Sclean = State(P, lse, edge, True), State(P, lse, edge, False), State(P, lse, edge, False)
    run_fused(L, Sg, table, mc)
    run_fused(FK, Sc, table, mc)
    run_fused(FK, Sclean, clean, mc)
    got, want, ref = Sg.out(), Sc.out(), Sclean.out()
    assert got["flags"] == want["flags"] == 1 and ref["flags"] == 0
    np.testing.assert_array_equal(want["cnt"], ref["cnt"])
    check_state(got, want, P, 0)
    for g, f, s in fold_rows(P, want):
        assert got["lse"][g] == want["lse"][g], (g, f, s, got["lse"][g], want["lse"][g])
    assert (got["lse"][rows] == 1.0e30).all()
    assert int(want["cnt"][2 * B + s16]) > 0                      # the search went on past the poisoned cell


# ------------------------------------------------------------------ candidates
CAND_C = [1, 64, 65, 255, 256, 257, 511, 512, 513, 768, 769, 1024]
# a sentence plants its winner at one index, or a tie at a pair of indices (the lower must win): the ends of a lane's row, of each group
# of 4 x 64 and of the eight-candidate batches (512, 1 024)
PLANTS = [(0,), ("last",), (63, 64), (255, 256), (256, 257), (511, 512), (512, 513), (767, 768), (768, 769), (0, "last"), (1022, 1023)]


def cand_problem(C):
    """beam 1: frame 1 a cell of 2 nodes, frame 2 one of C nodes = C candidates"""
    P = lattice(1, [cells([2, C], mix_last=False) for _ in PLANTS])
    lse, edge = dyadic_inputs(P, 100 + C)
    for s, at in enumerate(PLANTS):
        idx = [C - 1 if a == "last" else a for a in at]
        if all(c < C for c in idx):
            for c in idx:
                plant(P, edge, 2, s, c, 64.0)
    return P, lse, edge


@gpu
@pytest.mark.parametrize("C", CAND_C)
def test_candidate_counts(L, C):
    """every C at which the batches of eight change path; == the reference row by row, the planted winner (the lower index of a tie) first"""
    P, lse, edge = cand_problem(C)
    _, want = compare(L, P, 0, lse, edge, backtrace=True, expect="ONE_PIECE")
    for s, at in enumerate(PLANTS):
        idx = [C - 1 if a == "last" else a for a in at]
        if all(c < C for c in idx):
            assert int(want["node"][2 * P["rmax"] + s]) - nb_of(P, 2, s) == min(idx), (s, at)


TIE_BEAM, TIE_NODES = 3, 342                                     # C = 1 026 = 16 x 64 + 2
TIE_GROUPS = [[254, 255, 256, 257, 258], [510, 511, 512, 513, 514], [766, 767, 768, 769, 770], [1021, 1022, 1023, 1024, 1025],
              [7 + 64 * j for j in (3, 4, 7, 8, 11, 12)],        # one lane: across its groups of 4 and the register / LDS line
              [63 + 64 * 7, 64 * 8, 63 + 64 * 11, 64 * 12, 63 + 64 * 15, 64 * 16],
              list(range(TIE_BEAM * TIE_NODES))]


@gpu
def test_ties_at_group_boundaries(L):
    """beam 3, more candidates tied at the best key than free ranks (test_gpu_beam_forms.py::tie_problem at C = 1 026): the survivors are the
    lowest candidate indices, in index order"""
    beam = TIE_BEAM
    P = lattice(beam, [cells([4, TIE_NODES], mix_last=False) for _ in TIE_GROUPS])
    lse, edge = dyadic_inputs(P, 34)
    rmax = P["rmax"]
    for s, grp in enumerate(TIE_GROUPS):
        nb1 = nb_of(P, 1, s)
        for j in range(4):
            edge[(nb1 + j) * beam] = -0.5 * j if j < 3 else -10.0
        for k in range(beam):
            lse[rmax + s * beam + k] = 8.125 - 0.5 * k               # score + lse the same for every predecessor
        for c in grp:
            plant(P, edge, 2, s, c, 20.0)
    _, want = compare(L, P, 0, lse, edge, expect="ONE_PIECE")
    for s, grp in enumerate(TIE_GROUPS):
        g = 2 * rmax + s * beam
        won = [(int(want["node"][g + r]) - nb_of(P, 2, s)) * beam + int(want["bp"][g + r]) - (rmax + s * beam) for r in range(beam)]
        assert won == sorted(grp)[:beam], (s, won)
        assert len(set(want["score"][g:g + beam])) == 1


# ------------------------------------------------------------------ reused buffers, fused
@gpu
def test_reused_buffers_fused(L):
    """two problems back to back on the same device buffers, fused (33 slices), as a decode plan serves its batches: only cnt, n_live and
    the flag word are zeroed between them; before the first run bp / node / word / score hold INT32 extremes and NaN"""
    beam, F, n_parts = 10, 6, 33
    P1 = lattice(beam, [cells([7, 9, 60, 4, 6]), cells([10, 3, 2]), cells([6, 14, 3, 3, 9]), cells([9])], F)
    P2 = lattice(beam, [cells([6, 2]), cells([5, 11, 70, 2, 3]), cells([8]), cells([10, 4, 13, 6])], F)
    mc = (max(P1["max_cands"], P2["max_cands"]) + 255) // 256 * 256
    step_form(L, P1, 0, mc)
    in1, in2 = dyadic_inputs(P1, 61), dyadic_inputs(P2, 62)
    n_edge = max(len(in1[1]), len(in2[1]))
    blank = np.full(P1["G"], 1.0e30)
    Sg = State(P1, blank, in1[1], True, fill=True, n_edge=n_edge)
    run_fused(L, Sg, exact_table(P1, n_parts), mc)
    Sc1 = State(P1, blank, in1[1], False)
    run_fused(FK, Sc1, exact_table(P1, n_parts), mc)
    check_state(Sg.out(), Sc1.out(), P1, 0)
    Sg.cnt.zero_(); Sg.n_live.zero_(); Sg.flags.zero_()
    Sg.edge[:len(in2[1])].copy_(Sg.t(in2[1]))
    Sg.set_lattice(P2)
    run_fused(L, Sg, exact_table(P2, n_parts) + np.float32(0.0), mc)
    Sc = State(P2, blank, in2[1], False)
    run_fused(FK, Sc, exact_table(P2, n_parts), mc)
    got, want = Sg.out(), Sc.out()
    assert got["flags"] == want["flags"] == 0
    check_state(got, want, P2, 0)
    for g, _f, _s in fold_rows(P2, want):
        assert got["lse"][g] == want["lse"][g] == 3.0 + g % 5
    check_backtrace(L, Sg, Sc, P2["F"] + 1)
