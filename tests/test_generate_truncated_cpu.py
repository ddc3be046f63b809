"""CPU-only: top-k / nucleus truncation of the sampler (jlm_amd/generate.py) -- the numpy rule ``kept_mask``, the argument checks, the
CLI flags, and the plumbing from ``LSTM_Model.generate`` to the op, through a numpy double of the two generate ops that draws from
the oracle's logits (tests/fake_hip.py's FakeOps has neither op: the double below adds both).  Also the condition the GPU kernel test
leans on: none of its cuts lies within the excuse distance of a boundary, so its cap on excused draws cannot hide a wrong cut."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
from jlm_amd import _lib, generate as G, ops as _ops                                     # noqa: E402
from tests import fake_hip, truncated_rows as TR                                          # noqa: E402
from tests.gpu_rows import load_model, lse, oracle_lm, ragged_prompts                     # noqa: E402


# ------------------------------------------------------------------------------------------------------------- kept_mask
def _rows():
    rng = np.random.RandomState(0)
    rows = [(rng.standard_normal(n) * 3).astype(np.float32) for n in (1, 2, 7, 64, 301)]
    tied = rng.choice([-1.5, 0.0, 0.25, 2.0], size=97).astype(np.float32)              # exact ties everywhere
    tied[[3, 40, 41]] = -0.0                                                              # -0 ranks with +0
    return rows + [tied, np.full(33, 1.25, dtype=np.float32)]


@pytest.mark.parametrize("temperature", [0.05, 1.0, 10.0])
def test_kept_mask_properties(temperature):
    for y in _rows():
        V = len(y)
        top = int(np.argmax(y))
        one = G.kept_mask(y, temperature, top_k=1)
        assert one.sum() == 1 and one[top]                                               # the argmax, the lowest id on a tie
        assert G.kept_mask(y, temperature, top_p=1e-9).nonzero()[0].tolist() == [top]    # p tiny: exactly one word
        assert G.kept_mask(y, temperature, top_k=V + 5, top_p=1.0).all() and G.kept_mask(y, temperature).all()
        ks = [G.kept_mask(y, temperature, top_k=k) for k in range(1, V + 1)]
        for k, (a, b) in enumerate(zip(ks, ks[1:]), start=1):
            assert a.sum() == k and not (a & ~b).any()                                   # kept(k1) within kept(k2)
        ps = [G.kept_mask(y, temperature, top_p=p) for p in (1e-6, 0.1, 0.5, 0.9, 0.999, 1.0)]
        for a, b in zip(ps, ps[1:]):
            assert a.sum() >= 1 and not (a & ~b).any()                                   # kept(p1) within kept(p2)
        # a kept set is a prefix of the rank order: nothing outside it outranks anything inside
        order = TR.rank_order(y)
        for m in ks[:5] + ps:
            assert m[order[:m.sum()]].all()


def test_kept_mask_top_k_before_top_p():
    y = np.log(np.array([0.4, 0.3, 0.2, 0.1])).astype(np.float32)
    # p alone: 0.4 + 0.3 = 0.7 < 0.75, a third word is needed
    assert G.kept_mask(y, 1.0, top_p=0.75).tolist() == [True, True, True, False]
    # after top-k = 2 the mass is 0.7, and 0.4 < 0.75 * 0.7 = 0.525 <= 0.7: both stay.  After top-k = 3 it is 0.9, and
    # 0.75 * 0.9 = 0.675 <= 0.7 keeps two words where p of the full mass kept three: top-k comes first
    assert G.kept_mask(y, 1.0, top_k=2, top_p=0.75).tolist() == [True, True, False, False]
    assert G.kept_mask(y, 1.0, top_k=3, top_p=0.75).tolist() == [True, True, False, False]
    # top-p never adds to what top-k kept
    assert G.kept_mask(y, 1.0, top_k=1, top_p=0.99).tolist() == [True, False, False, False]


def test_kept_mask_ties_at_the_cut_go_by_id():
    y = np.array([1.0, 3.0, 1.0, 2.0, 1.0, 1.0, 0.5], dtype=np.float32)
    assert G.kept_mask(y, 1.0, top_k=3).nonzero()[0].tolist() == [0, 1, 3]               # one of the four 1.0s: the lowest id
    assert G.kept_mask(y, 1.0, top_k=4).nonzero()[0].tolist() == [0, 1, 2, 3]
    eq = np.full(9, -2.0, dtype=np.float32)
    assert G.kept_mask(eq, 0.7, top_k=4).nonzero()[0].tolist() == [0, 1, 2, 3]
    assert G.kept_mask(eq, 0.7, top_p=0.5).nonzero()[0].tolist() == [0, 1, 2, 3, 4]      # 4 / 9 < 0.5 <= 5 / 9
    # the rank order is of the logits: the temperature moves a top-p cut, never a top-k one
    y = (np.random.RandomState(1).standard_normal(50) * 2).astype(np.float32)
    assert np.array_equal(G.kept_mask(y, 0.05, top_k=7), G.kept_mask(y, 10.0, top_k=7))
    assert G.kept_mask(y, 0.05, top_p=0.9).sum() < G.kept_mask(y, 10.0, top_p=0.9).sum()
    # temperature 0 is greedy whatever k and p are
    assert G.kept_mask(y, 0.0, top_k=7, top_p=0.9).nonzero()[0].tolist() == [int(np.argmax(y))]


# ------------------------------------------------------------------------------------------------------------- arguments, CLI
@pytest.mark.parametrize("kw", [dict(top_k=0), dict(top_k=-3), dict(top_k=True), dict(top_k=2.0), dict(top_k="4"),
                                dict(top_p=0.0), dict(top_p=-0.1), dict(top_p=1.0001), dict(top_p=float("nan")), dict(top_p=float("inf")),
                                dict(top_p=True), dict(top_p="x")])
def test_truncation_argument_errors(kw):
    with pytest.raises(ValueError, match="top_k|top_p"):
        G.check_args([[1, 2]], 3, 1.0, 0, None, 20, **kw)
    with pytest.raises(ValueError):
        G.check_truncation(kw.get("top_k"), kw.get("top_p"), 20)


def test_truncation_off_values_become_none():
    assert G.check_truncation(None, None, 20) == (None, None)
    assert G.check_truncation(20, 1.0, 20) == (None, None)
    assert G.check_truncation(10 ** 9, 1, 20) == (None, None)
    assert G.check_truncation(np.int64(19), np.float32(0.5), 20) == (19, 0.5)
    assert G.check_truncation(1, 1e-300, 20) == (1, 1e-300)
    assert G.check_args([[3]], 2, 1.0, 0, None, 20, 5, 0.5)[0].tolist() == [3]           # what check_args returns is unchanged


def test_lib_exposes_the_truncated_entries():
    assert "jlm_sample_rows_trunc" in _lib.EXPORTS and "jlm_generate_frames_trunc" in _lib.EXPORTS
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "jlm_sample_rows_trunc") and hasattr(lib, "jlm_generate_frames_trunc")
    assert lib.jlm_abi_version() == 12


# ------------------------------------------------------------------------------------------------------------- plumbing
class OracleOps(fake_hip.FakeOps):
    """FakeOps with the two generate ops drawn from the oracle's float64 logits (cast to f32, as the device materialises them) by the
    numpy rule.  ``calls`` records (op name, number of arguments, top_k, top_p)."""

    def __init__(self, lib, lm):
        super().__init__(lib)
        self.lm, self.calls = lm, []

    def generate_frames(self, *a):
        assert len(a) == 26                               # the op's signature, unchanged
        self.calls.append(("generate_frames", len(a), None, None))
        return self._run(a, None, None)

    def generate_frames_trunc(self, *a):
        assert len(a) == 28
        top_k, top_p = a[26], a[27]
        assert isinstance(top_k, int) and isinstance(top_p, float)
        self.calls.append(("generate_frames_trunc", len(a), top_k, top_p))
        return self._run(a[:26], top_k if top_k > 0 else None, top_p if top_p < 1 else None)

    def _run(self, a, top_k, top_p):
        (_model, _h0, _c0, _h1, _c1, _T, _logits, _ld, _rows, _prev, prompt, _n_live, n_live_host, row_id, word, done, stop_id,
         temperature, seed, ids, nll, _flags, R, P, N, timed) = a
        assert not timed
        lm, sn = self.lm, self.lm.config["self_norm"]
        prompt, row_id = prompt.numpy().reshape(P, R), row_id.numpy()
        ids, nll = ids.numpy().reshape(N, R), nll.numpy().reshape(N, R)                 # views: written in place
        for r in range(R):
            h, c = lm.zero_state(1)
            for f in range(P):
                if r < n_live_host[f]:                    # right-aligned prompts: the rows live at frame f are a prefix
                    h, c = lm.lstm_cell(np.array([prompt[f, r]]), h, c)
            for k in range(N):
                y = lm.project(h)[0]
                y32 = y.astype(np.float32)
                if temperature == 0:
                    w = int(np.argmax(y32))
                else:
                    keep = G.kept_mask(y32, temperature, top_k, top_p)
                    w = G.inverse_cdf(np.where(keep, TR.masses(y32, temperature), 0.0), float(G.uniform(seed & (2 ** 64 - 1), k, row_id[r])))
                ids[k, r] = w
                nll[k, r] = -y[w] if sn else lse(y) - y[w]
                word[r] = w
                if done is not None and w == stop_id:
                    done[r] = 1
                    break
                h, c = lm.lstm_cell(np.array([w]), h, c)
        return torch.empty(0, dtype=torch.float64)


@pytest.fixture
def oracle_model(fx, monkeypatch):
    def make(name):
        f = fx(name)
        fake = fake_hip.install(monkeypatch)
        ops = OracleOps(fake, oracle_lm(f["root"]))
        monkeypatch.setattr(_ops, "_backend", ops)
        return f, load_model(f["root"]), ops
    return make


def test_untruncated_calls_reach_the_old_op_unchanged(oracle_model):
    f, model, ops = oracle_model("small-vtable")
    V = model.dev.V
    prompts = ragged_prompts(9, V, seed=4)
    ids, nll = model.generate(prompts, 6, temperature=0.9, seed=11)
    assert ops.calls and all(c == ("generate_frames", 26, None, None) for c in ops.calls)
    n = len(ops.calls)
    # "off" spelled out: the same op, the same draws
    for kw in (dict(top_k=None, top_p=None), dict(top_k=V, top_p=1.0), dict(top_k=V + 7), dict(top_p=1)):
        ids2, nll2 = model.generate(prompts, 6, temperature=0.9, seed=11, **kw)
        for a, b, c, d in zip(ids, ids2, nll, nll2):
            assert np.array_equal(a, b) and np.array_equal(c, d)
    assert len(ops.calls) > n and all(c[0] == "generate_frames" for c in ops.calls)
    agree, excused, _ = TR.oracle_follow(ops.lm, prompts, ids, 0.9, 11, None, None, 1e-6)
    assert excused == 0 and agree == 9 * 6


@pytest.mark.parametrize("name", ["small-vtable", "small-char"])
def test_truncated_calls_draw_from_the_kept_set(name, oracle_model):
    f, model, ops = oracle_model(name)
    V = model.dev.V
    prompts = ragged_prompts(11, V, seed=5)
    ids, nll = model.generate(prompts, 7, temperature=1.3, seed=2 ** 64 - 9, top_k=5, top_p=0.7)
    assert [c[0] for c in ops.calls] == ["generate_frames_trunc"] and ops.calls[0][2:] == (5, 0.7)
    # every draw lies in the oracle's kept set and is the restricted inverse-CDF draw (the f32 cast of the double's logits moves a
    # mass by ~1e-7 of itself: 1e-6 excuses a draw that close to a boundary, and none is expected)
    agree, excused, onll = TR.oracle_follow(ops.lm, prompts, ids, 1.3, 2 ** 64 - 9, 5, 0.7, 1e-6)
    assert excused == 0 and agree == 11 * 7
    lm = ops.lm
    for r, (p, x) in enumerate(zip(prompts, ids)):
        h, c = lm.zero_state(1)
        for w in p:
            h, c = lm.lstm_cell(np.array([w]), h, c)
        for w in x:
            keep = G.kept_mask(lm.project(h)[0], 1.3, 5, 0.7)
            assert keep[w] and keep.sum() <= 5
            h, c = lm.lstm_cell(np.array([w]), h, c)
        np.testing.assert_allclose(nll[r], onll[r], rtol=0, atol=1e-12)                 # the nll of the FULL distribution
    # the same rows cut into several calls: the same draws
    ops.calls.clear()
    ids2, nll2 = model.generate(prompts, 7, temperature=1.3, seed=2 ** 64 - 9, top_k=5, top_p=0.7, max_rows=4)
    assert len(ops.calls) == 3 and all(c == ("generate_frames_trunc", 28, 5, 0.7) for c in ops.calls)
    for a, b, c, d in zip(ids, ids2, nll, nll2):
        assert np.array_equal(a, b) and np.array_equal(c, d)
    # one knob at a time: the other travels as "off"
    ops.calls.clear()
    model.generate(prompts[:2], 2, top_k=3)
    model.generate(prompts[:2], 2, top_p=0.25)
    assert [c[2:] for c in ops.calls] == [(3, 1.0), (0, 0.25)]
    # a bad knob raises before any op runs
    ops.calls.clear()
    for kw in (dict(top_k=0), dict(top_p=0.0), dict(top_p=1.5), dict(top_k=1.5)):
        with pytest.raises(ValueError):
            model.generate(prompts, 3, **kw)
    assert not ops.calls


def test_cli_flags_reach_the_op(oracle_model, capsys):
    f, _model, ops = oracle_model("small-vtable")
    ids, nll = G.main(["--root", f["root"], "-e", "1", "-n", "4", "--words", "5", "--top-k", "5", "--top-p", "0.8", "--show-nll"])
    assert [c[2:] for c in ops.calls] == [(5, 0.8)]
    lines = [l for l in capsys.readouterr().out.strip().split("\n") if not l.startswith("LSTM model:")]
    assert len(lines) == 4 and all(len(x) == 5 for x in ids)
    for line, l in zip(lines, nll):
        assert abs(float(line.split("\t")[1]) - l.sum()) < 1e-3
    ops.calls.clear()
    G.main(["--root", f["root"], "-e", "1", "--words", "2"])
    assert [c[0] for c in ops.calls] == ["generate_frames"]
    with pytest.raises(SystemExit):
        G.main(["--root", f["root"], "-e", "1", "--top-k", "1.5"])


# ------------------------------------------------------------------------------------------------------------- the GPU test's cuts
def test_kernel_test_cuts_are_unambiguous():
    """For every row, temperature and (k, p) with p < 1 of the GPU kernel test, p S_K stays further than a relative 1e-9 from every
    boundary of the rank-order cumulative mass: the kernel's cut must equal kept_mask's in every one of them."""
    cases, nearest = 0, 1.0
    for n_cols in TR.N_COLS:
        y = TR.kernel_logits(n_cols)
        orders = [TR.rank_order(row) for row in y]
        for temperature in TR.TEMPERATURES:
            for row, order in zip(y, orders):
                ranked = TR.masses(row, temperature)[order]
                for k, p in TR.KP:
                    if p is None or p >= 1:
                        continue
                    d = TR.cut_distance(ranked[:n_cols if k is None else min(k, n_cols)], p)
                    assert d > TR.TOL_KERNEL, (n_cols, temperature, k, p, d)
                    nearest = min(nearest, d)
                    cases += 1
    assert cases == 6048
    print("cuts checked: %d, nearest %.3g" % (cases, nearest))
