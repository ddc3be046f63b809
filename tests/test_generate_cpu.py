"""CPU-only: the host side of batched sampling (jlm_amd/generate.py) -- the counter-based random numbers, the inverse-CDF and greedy
rules the kernel implements (restated in numpy), the row plan, prompt alignment, stop truncation, argument checks, and the new C
entry points in the ctypes table."""
import ctypes

import numpy as np
import pytest

from jlm_amd import _lib, generate as G


def _u_int(seed, step, row):
    """the generator restated with Python integers (include/jlm_hip.h jlm_sample_rows)"""
    M = (1 << 64) - 1
    z = (seed + 0x9E3779B97F4A7C15 * ((step << 32) | (row + 1))) & M
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
    z ^= z >> 31
    return ((z >> 11) + 0.5) * 2.0 ** -53


PINNED = [((0, 0, 0), 0.8833108082136427), ((0, 0, 1), 0.43152799704851), ((0, 1, 0), 0.2735784634770609),
          ((12345, 7, 2559), 0.3455905656267761)]


@pytest.mark.parametrize("args,want", PINNED)
def test_uniform_pinned_values(args, want):
    assert G.uniform(*args) == want
    assert _u_int(*args) == want


def test_uniform_vectorised_matches_integer_form():
    rng = np.random.RandomState(1)
    for seed in (0, 1, 2 ** 63, 2 ** 64 - 1, 987654321):
        steps = rng.randint(0, 5000, size=50)
        rows = rng.randint(0, 70000, size=50)
        got = G.uniform(seed, steps, rows)
        assert np.all((got > 0) & (got < 1))
        for s, r, g in zip(steps, rows, got):
            assert g == _u_int(seed, int(s), int(r))


def test_inverse_cdf_rule():
    mass = np.array([0.0, 1.0, 0.0, 2.0, 1.0])          # cumsum 0 1 1 3 4
    assert G.inverse_cdf(mass, 0.0) == 1                 # the smallest i with cumsum > u S: a word with mass
    assert G.inverse_cdf(mass, 0.2499) == 1
    assert G.inverse_cdf(mass, 0.25) == 3                # cumsum == u S is not a crossing
    assert G.inverse_cdf(mass, 0.75) == 4
    assert G.inverse_cdf(mass, 1.0) == 4                 # no crossing: the last word with non-zero mass
    assert G.inverse_cdf(np.array([1.0, 1.0, 0.0, 0.0]), 1.0) == 1


def test_greedy_tie_rule_is_lowest_id():
    y = np.array([0.5, 3.0, -1.0, 3.0, 3.0], dtype=np.float32)
    assert int(np.argmax(y)) == 1                        # what the kernel's greedy draw pins


def test_plan_rows_prefix_and_cuts():
    lens = [2, 5, 1, 5, 3, 1, 4]
    chunks = G.plan_rows(lens, 3)
    assert [list(c["idx"]) for c in chunks] == [[1, 3, 6], [4, 0, 2], [5]]
    for c in chunks:
        P = c["n_prompt"]
        assert P == c["lens"].max()
        # rows live at prompt frame f are those whose right-aligned prompt has started: a prefix, all rows at the last frame
        for f in range(P):
            live = c["lens"] >= P - f
            assert live.sum() == c["n_live"][f]
            assert np.all(live[:c["n_live"][f]])
        assert c["n_live"][-1] == len(c["idx"])
    with pytest.raises(ValueError):
        G.plan_rows(lens, 0)


def test_prompt_arrays_right_aligned():
    prompt, prev = G.prompt_arrays([[5, 6, 7], [8, 9], [4]], 3)
    assert prompt.tolist() == [[5, 0, 0], [6, 8, 0], [7, 9, 4]]
    # -1 (zero state) at each row's first frame, the row itself after it
    assert prev[:, 0].tolist() == [-1, 0, 0]
    assert prev[:, 1].tolist() == [-1, -1, 1]
    assert prev[:, 2].tolist() == [-1, -1, -1]


def test_random_numbers_independent_of_the_cut():
    """the (step, row) of every draw is the caller's row index, whatever chunk the row lands in: every cut of the same rows asks for
    the same u's"""
    lens = np.random.RandomState(3).randint(1, 9, size=23)
    n_words = 4

    def us(max_rows):
        out = {}
        for c in G.plan_rows(lens, max_rows):
            for r in c["idx"]:
                out[int(r)] = G.uniform(99, np.arange(n_words), int(r))
        return out

    a, b = us(23), us(5)
    assert sorted(a) == list(range(23))
    for r in a:
        assert np.array_equal(a[r], b[r])


def test_truncate_at_stop():
    ids = np.array([4, 7, 2, 7, 1])
    assert G.truncate(ids, 7).tolist() == [4, 7]
    assert G.truncate(ids, 9).tolist() == [4, 7, 2, 7, 1]
    assert G.truncate(ids, None).tolist() == [4, 7, 2, 7, 1]
    assert G.truncate(np.array([3]), 3).tolist() == [3]


@pytest.mark.parametrize("kw,match", [
    (dict(prompts=[[1, 2], []]), "empty"),
    (dict(prompts=[[1, 20]]), "outside"),
    (dict(prompts=[[-1]]), "outside"),
    (dict(n_words=-1), "n_words"),
    (dict(n_words=2.5), "n_words"),
    (dict(temperature=-0.5), "temperature"),
    (dict(temperature=float("nan")), "temperature"),
    (dict(temperature=float("inf")), "temperature"),
    (dict(seed=-1), "seed"),
    (dict(seed=2 ** 64), "seed"),
    (dict(stop_id=20), "outside"),
])
def test_argument_errors(kw, match):
    args = dict(prompts=[[1, 2]], n_words=3, temperature=1.0, seed=0, stop_id=None, V=20)
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        G.check_args(**args)


def test_default_prompt_is_eos():
    p = G.check_args(None, 5, 1.0, 0, None, 20)
    assert [list(x) for x in p] == [[G.EOS_ID]]
    assert G.check_args([[3]], 0, 0.0, 2 ** 64 - 1, 3, 20)[0].tolist() == [3]


def test_lib_exposes_the_sampling_entries():
    assert "jlm_sample_rows" in _lib.EXPORTS and "jlm_generate_frames" in _lib.EXPORTS
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "jlm_sample_rows") and hasattr(lib, "jlm_generate_frames")
    names = [f[0] for f in _lib.GeneratePlan._fields_]
    assert names[:3] == ["n_rows", "n_prompt", "n_words"] and "seed" in names and "temperature" in names
