"""CPU-only: the stage-wise error decomposition of tests/score_budget.py on a stand-in "device" -- the float64 oracle on wide-vtable
with its state, log-normaliser and target logit rounded to f32 every step (score_budget.stand_in_steps).  The identities hold; the
bias test |mean| <= 4 rms / sqrt(N) stays quiet on the reference alone and speaks, in the right stage only, when an error is planted:
a common-mode h (1 + 2^-24) after every step in `gate` (and a same-signed `drift`), a rounding of T to f32 in `tproj`.

The planted bias moves a token's nll by (E_p[y_T] - y_T(target)) 2^-24.  wide-vtable's logits are flat, so with random targets that
factor is small and of either sign: the plant then gives `gate` a mean of 1.0e-10 against 4 rms / sqrt(N) = 3.8e-10 over 1 600 tokens,
which nothing can tell from none (it would take 22 000 tokens).  The bias case therefore scores every sentence on the word the oracle
finds LEAST likely, where the factor has one sign on every token (mean 7.0e-9 against 7.3e-10) -- as logits of +-20 give it with
random targets on the device (tests/test_gpu_score_budget.py) -- and runs the same sentences without the plant as its control."""
import numpy as np
import pytest

from oracle import jlm_oracle as orc
from tests import score_budget as sb

R, LO, HI = 48, 28, 39


@pytest.fixture(scope="module")
def lm(fx):
    return orc.OracleDecoder(fx("wide-vtable")["root"], 1).model


@pytest.fixture(scope="module")
def case(lm):
    """random targets"""
    rng = np.random.RandomState(17)
    V = lm.weights["b2"].shape[0]
    seqs = [list(rng.randint(1, V, size=L)) for L in rng.randint(LO, HI + 1, size=R)]
    return (lm,) + sb.sentence_steps(seqs, 1)


@pytest.fixture(scope="module")
def unlikely(lm):
    """every next word the oracle's least likely one"""
    lens = np.random.RandomState(18).randint(LO, HI + 1, size=R)
    start = np.arange(1, R + 1)                                            # (distinct first words: distinct sentences)
    seqs = sb.chosen_sentences(lm, start, lens, np.argmin)
    x, y, lens = sb.sentence_steps(seqs, 1)
    x[:, 0] = start
    return lm, x, y, lens


def _budget(case, **plant):
    lm, x, y, lens = case
    return sb.decompose(lm, sb.stand_in_steps(lm, x, y, lens, **plant))             # (asserts the two identities)


def test_layout_and_projection_agree_with_the_oracle(case):
    lm, x, _y, _lens = case
    h = sb.oracle_run(lm, x[:, :3]).reshape(-1, lm.hidden_size)
    offs, ldt = sb.t_layout(lm)
    assert [s for _o, s in offs] == [s[0] for s in lm.segs] and ldt == sum((s[0] + 3) // 4 * 4 for s in lm.segs)
    np.testing.assert_allclose(sb.logits_from_T(lm, sb.oracle_T(lm, h)), lm.project(h), rtol=0, atol=1e-12)


def test_sentence_steps_are_the_scorers(case):
    from jlm_amd.score import sentence_arrays
    _lm, x, y, lens = case
    seqs = [y[r, :lens[r]] for r in range(len(lens))]
    word, target = sentence_arrays(seqs, 1, x.shape[1])
    for r, L in enumerate(lens):
        assert (x[r, :L] == word[:L, r]).all() and (y[r, :L] == target[:L, r]).all()


def test_without_a_plant_every_stage_is_unbiased(case):
    b = _budget(case)
    print(sb.table("stand-in, no plant", b))
    assert len(b.total) == case[3].sum() and b.n_rows == R
    for s in sb.LOCAL:
        ok, mean, bar = sb.unbiased(b.dev[s])
        assert ok, (s, mean, bar)
    assert (np.abs(b.dev["logit"]) <= b.bound).all()                                # (a correctly rounded logit is inside the chain's bound)


def test_a_common_mode_bias_of_h_shows_in_gate_and_nowhere_else(unlikely):
    clean, b = _budget(unlikely), _budget(unlikely, h_bias=2.0 ** -24)
    print(sb.table("stand-in, least likely targets, no plant", clean))
    print(sb.table("stand-in, least likely targets, h (1 + 2^-24) after every step", b))
    for s in sb.LOCAL:
        ok, mean, bar = sb.unbiased(clean.dev[s])
        assert ok, ("no plant", s, mean, bar)
    ok, mean, bar = sb.unbiased(b.dev["gate"])
    assert not ok and abs(mean) > bar, ("gate", mean, bar)
    for s in ("tproj", "norm", "logit"):
        ok, mean, bar = sb.unbiased(b.dev[s])
        assert ok, (s, mean, bar)
    # the drift it leaves is same-signed: its mean is many standard errors from 0, and the sentences' sums all carry that sign
    ok, mean, bar = sb.unbiased(b.dev["drift"])
    assert not ok, ("drift", mean, bar)
    sums = b.sentence_sums(b.dev["drift"])
    assert (np.sign(sums) == np.sign(mean)).mean() >= 0.9, sums
    assert abs(mean) > 4 * abs(clean.dev["drift"].mean())


def test_a_rounding_of_T_shows_in_tproj_only(case):
    clean, b = _budget(case), _budget(case, round_T=True)
    print(sb.table("stand-in, T rounded to f32", b))
    rms = lambda e: float(np.sqrt(np.mean(e * e)))
    assert rms(b.dev["tproj"]) > 1e3 * rms(clean.dev["tproj"]) and rms(b.dev["tproj"]) > 1e-9
    # the state does not see T: the other stages are what they were, to the bit (norm and logit up to the f32 rounding of other values)
    for s in ("drift", "gate"):
        assert np.array_equal(b.dev[s], clean.dev[s]), s
    for s in ("norm", "logit"):
        assert rms(b.dev[s]) <= 1.5 * rms(clean.dev[s]) + 1e-12, s
        assert sb.unbiased(b.dev[s])[0], s
    assert sb.unbiased(b.dev["tproj"])[0]                                           # (a rounding is no bias)
