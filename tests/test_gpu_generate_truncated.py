"""GPU: top-k / nucleus sampling (LSTM_Model.generate(top_k=, top_p=), python -m jlm_amd.generate --top-k --top-p; csrc
jlm_generate_frames_trunc + sample_rows_trunc_kernel).

Kernel level (torch.ops.jlm.sample_rows_trunc over logits the test writes): every draw lies in ``generate.kept_mask``'s set and is
the float64 inverse CDF over it with the same u.  A draw is excused, and counted, only where u S_kept or p S_K lies within a relative
1e-9 of a boundary -- the bar of tests/test_gpu_generate.py's draw test, for the same reason: f32 expf terms, f64 (here also exact
fixed-point) sums.  tests/test_generate_truncated_cpu.py shows no cut of the random cases is that close, so those cuts are exact.

End to end, against the oracle's float64 OracleLM teacher-forced on the device's draws, with the existing end-to-end tolerance
TOL_E2E for a boundary (of the kept CDF, of the rank-order cumulative mass, or between the logits at ranks k and k + 1)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
from jlm_amd import _lib, generate as G, ops as _ops                                     # noqa: E402
from tests import truncated_rows as TR                                                   # noqa: E402
from tests.gpu_rows import load_model, lse, oracle_lm, ragged_prompts                    # noqa: E402
from tests.test_gpu_generate import TOK_ATOL, TOL_E2E, _chi2_sf_wh, _sample, _samples    # noqa: E402

pytestmark = pytest.mark.gpu


class Rows:
    """logits y [R, n_cols] (f32 numpy) on the device, padded to the kernel's row stride with NaN (never read as a word)"""

    def __init__(self, y):
        self.dev = _lib.require_gpu()
        self.y = y
        self.R, self.n = y.shape
        self.ld = (self.n + 3) // 4 * 4
        yp = np.full((self.R, self.ld), np.nan, dtype=np.float32)
        yp[:, :self.n] = y
        self.yt = torch.from_numpy(yp).to(self.dev)

    def sample(self, temperature, seed, step, top_k=None, top_p=None, row_id=None, forced=None, done=None, stop_id=-1, self_norm=False,
               n_dev=None, word0=None):
        """one jlm_sample_rows_trunc launch -> (ids, nll, word, flags, done)"""
        it = lambda a: None if a is None else torch.as_tensor(np.asarray(a, dtype=np.int32)).to(self.dev)
        word = it(np.zeros(self.R) if word0 is None else word0)
        ids = torch.full((self.R,), -7, device=self.dev, dtype=torch.int32)
        nll = torch.zeros(self.R, device=self.dev, dtype=torch.float64)
        flags = torch.zeros(1, device=self.dev, dtype=torch.int32)
        dn = it(done)
        _ops.backend().sample_rows_trunc(self.yt, self.ld, self.n, self.R, it(n_dev), float(temperature), int(seed), int(step), it(row_id),
                                         it(forced), dn, int(stop_id), bool(self_norm), 0 if top_k is None else int(top_k),
                                         1.0 if top_p is None else float(top_p), word, ids, nll, flags)
        torch.cuda.synchronize()
        return ids.cpu().numpy(), nll.cpu().numpy(), word.cpu().numpy(), int(flags.cpu()[0]), None if dn is None else dn.cpu().numpy()


def _kernel_case(y, temperature, kps, seed=5, steps=3, self_norm=False, allow_excused=True):
    """every (k, p) of `kps` over `steps` draws of every row of y; -> (draws, excused)"""
    rows = Rows(y)
    R, n = y.shape
    row_id = np.arange(R) * 3 + 11
    orders = [TR.rank_order(r) for r in y]
    mass = None if temperature == 0 else [TR.masses(r, temperature) for r in y]
    lses = [lse(r) for r in y]
    total = excused = 0
    for k, p in kps:
        k = n if k == "V" else k
        case_total = case_excused = 0
        for step in range(steps):
            ids, nll, word, fl, _ = rows.sample(temperature, seed, step, k, p, row_id=row_id, self_norm=self_norm)
            assert fl == 0
            assert np.array_equal(ids, word)
            u = G.uniform(seed, step, row_id)
            for r in range(R):
                ok = TR.judge_draw(y[r], temperature, k, p, float(u[r]), int(ids[r]), TR.TOL_KERNEL, order=orders[r],
                                   mass=None if mass is None else mass[r])
                assert ok or (temperature != 0 and k != 1), (k, p, step, r, int(ids[r]))   # k = 1, greedy: no exceptions
                case_excused += not ok
                want = -float(y[r, ids[r]]) if self_norm else lses[r] - float(y[r, ids[r]])
                assert abs(nll[r] - want) <= 1e-6, (k, p, r, nll[r], want)
                case_total += 1
            if k == n and p == 1.0:                      # both off: jlm_sample_rows' draws
                assert np.array_equal(ids, _sample(y, temperature, seed, step, row_id=row_id, self_norm=self_norm)[0])
        print("n_cols %d tau %g k %s p %s: %d draws, %d excused" % (n, temperature, k, p, case_total, case_excused))
        assert case_excused <= (max(1, case_total // 100) if allow_excused else 0), (k, p, case_excused, case_total)
        total += case_total
        excused += case_excused
    return total, excused


@pytest.mark.parametrize("n_cols", TR.N_COLS)
@pytest.mark.parametrize("temperature", TR.TEMPERATURES)
def test_sample_rows_trunc_random_logits(n_cols, temperature):
    _kernel_case(TR.kernel_logits(n_cols), temperature, TR.KP)


@pytest.mark.parametrize("n_cols", [65, 1025])
def test_sample_rows_trunc_greedy_whatever_k_and_p(n_cols):
    _kernel_case(TR.kernel_logits(n_cols), 0.0, TR.KP, steps=1, allow_excused=False)


def test_sample_rows_trunc_self_norm():
    y = (np.random.RandomState(8).standard_normal((32, 777)) * 2).astype(np.float32)
    _kernel_case(y, 1.0, [(1, None), (9, 0.8), (None, 0.3)], self_norm=True)
    _kernel_case(y, 0.0, [(9, 0.8)], self_norm=True, allow_excused=False)


def _kept(rows, temperature, top_k, top_p, seeds=range(40)):
    """the words each row draws over many seeds -> list of sets"""
    seen = [set() for _ in range(rows.R)]
    for seed in seeds:
        ids, _nll, _w, fl, _ = rows.sample(temperature, seed, 0, top_k, top_p)
        assert fl == 0
        for r, i in enumerate(ids):
            seen[r].add(int(i))
    return seen


@pytest.mark.parametrize("temperature", [0.05, 1.0, 10.0])
def test_sample_rows_trunc_special_rows(temperature):
    rng = np.random.RandomState(4)
    n = 5003
    # all-equal logits: both cuts are taken by id (5003 is odd, so p = 0.5 falls between two words: 2502 kept)
    eq = np.full((8, n), 1.25, dtype=np.float32)
    _kernel_case(eq, temperature, [(1, None), (7, None), (None, 0.5), (300, 0.101)], allow_excused=False)
    rows = Rows(eq)
    for r, seen in enumerate(_kept(rows, temperature, 7, None)):
        assert seen <= set(range(7)) and len(seen) >= 4, (r, seen)
    for seen in _kept(rows, temperature, None, 0.5, seeds=range(8)):
        assert max(seen) <= 2501
    ids = rows.sample(temperature, 1, 0, 300, 0.101)[0]                                 # 30.3 -> 31 equal masses: floor(31 u)
    assert np.array_equal(ids, np.floor(G.uniform(1, 0, np.arange(8)) * 31).astype(np.int64))
    # one dominant word with p = 0.9: exactly one word is kept
    dom = rng.standard_normal((8, n)).astype(np.float32)
    pos = rng.randint(0, n, size=8)
    dom[np.arange(8), pos] = 40.0
    _kernel_case(dom, temperature, [(None, 0.9), (40, 0.9), (3, None)])
    if temperature <= 1.0:                               # (at tau = 10 the other 5002 words hold most of the mass)
        assert all(G.kept_mask(dom[r], temperature, None, 0.9).sum() == 1 for r in range(8))
        for r, seen in enumerate(_kept(Rows(dom), temperature, None, 0.9, seeds=range(8))):
            assert seen == {int(pos[r])}
    # a tie straddling the k-th rank: ranks 3 .. 8 hold one value, k = 5 keeps the three lowest ids of them
    tie = rng.standard_normal((8, n)).astype(np.float32)
    tie[:, [10, 4000]] = [9.0, 8.0]
    tied = np.sort(rng.choice(np.arange(11, 3999), size=(8, 6)), axis=1)
    for r in range(8):
        tie[r, tied[r]] = 7.5
    _kernel_case(tie, temperature, [(5, None), (5, 0.999), (8, None), (9, None), (None, 0.5)], allow_excused=False)
    for r, seen in enumerate(_kept(Rows(tie), max(temperature, 1.0), 5, None, seeds=range(60))):
        assert seen <= {10, 4000} | set(tied[r, :3].tolist()), (r, seen)
    # logits of +-30, 2 500 of them +30 in every row: thousands of equal logits at the cut, and (tau <= 1) a tail whose mass
    # underflows to nothing beside the head's.  (The p's keep p S_K away from a whole number of head words.)
    pm = np.stack([rng.permutation(np.where(np.arange(n) < 2500, 30.0, -30.0)) for _ in range(8)]).astype(np.float32)
    _kernel_case(pm, temperature, [(100, None), (None, 0.2501), (4000, 0.9001), (None, 0.999999)], allow_excused=False)
    # a steep row at tau = 0.05: everything past the first few ranks underflows; the cut and the draw stay among words with mass
    steep = (rng.standard_normal((8, n)) * 30).astype(np.float32)
    _kernel_case(steep, temperature, [(40, None), (None, 0.9), (None, 0.999999), (2000, 0.5)])


def test_sample_rows_trunc_signed_zero_and_negative_logits():
    """-0 ranks with +0 (by id), and the rank order holds across the sign"""
    rng = np.random.RandomState(12)
    y = (rng.standard_normal((16, 515)) * 1e-3).astype(np.float32)
    y[:, ::5] = 0.0
    y[:, 1::10] = -0.0
    y[:, 7] = -np.inf                                    # a word of no mass is not an error
    _kernel_case(y, 1.0, [(1, None), (60, None), (150, None), (None, 0.3), (200, 0.6)], allow_excused=False)
    _kernel_case(-np.abs(y) - 1.0, 0.5, [(3, None), (None, 0.01)])


def test_sample_rows_trunc_nan_sets_flag():
    y = np.random.RandomState(2).standard_normal((4, 2000)).astype(np.float32)
    for bad in (np.nan, -np.nan, np.inf):
        y[2, 777] = bad
        for k, p in ((5, None), (None, 0.9), (1, None)):
            ids, _nll, word, fl, _ = Rows(y).sample(1.0, 0, 0, k, p)
            assert fl & 1
            assert ids[2] == -1 and 0 <= word[2] < 2000
            assert all(ids[r] >= 0 for r in (0, 1, 3))


def test_sample_rows_trunc_forced_done_and_live_count():
    rng = np.random.RandomState(9)
    y = rng.standard_normal((6, 300)).astype(np.float32)
    rows = Rows(y)
    forced = [-1, 17, -1, -1, -1, -1]
    done = [0, 0, 1, 0, 0, 0]
    ids, nll, word, fl, dn = rows.sample(1.0, 3, 2, 12, 0.9, forced=forced, done=done, stop_id=-1, n_dev=[5], word0=[9] * 6)
    assert fl == 0
    assert word[1] == 17 and ids[1] == -1 and nll[1] == 0    # forced: passes through
    assert ids[2] == -1 and word[2] == 9 and dn[2] == 1      # stopped: masked, its word kept
    assert ids[5] == -7 and word[5] == 9                     # past the live count: untouched
    u = G.uniform(3, 2, np.arange(6))
    for r in (0, 3, 4):
        assert ids[r] == word[r] >= 0
        assert TR.judge_draw(y[r], 1.0, 12, 0.9, float(u[r]), int(ids[r]), TR.TOL_KERNEL)
    # a draw of the stop word marks the row done
    ids2, _n, _w, _f, dn2 = rows.sample(1.0, 3, 2, 12, 0.9, done=[0] * 6, stop_id=int(ids[0]))
    assert dn2[0] == 1 and ids2[0] == ids[0]


def test_sample_rows_trunc_rejects_bad_top_p():
    rows = Rows(np.zeros((2, 8), dtype=np.float32))
    for p in (0.0, -1.0, float("nan")):
        with pytest.raises(RuntimeError):
            rows.sample(1.0, 0, 0, None, p)


# ------------------------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("name,top_k,top_p", [("small-tied", 5, 0.7), ("small-vtable", 8, None), ("small-vtable", None, 0.6),
                                              ("small-char", 6, 0.9), ("peaked20-vtable", 5, 0.8), ("small-tied-sn", 4, 0.5),
                                              # V = 2 003 cut at 501 / 1 203: unaligned segment columns, a partial last chunk
                                              ("odd-vtable", 8, 0.9), ("odd-vtable", None, 0.6), ("oddw-vtable", 5, 0.7),
                                              ("odd-tied", 6, None), ("odd-untied", 6, 0.8), ("odd-dsoftmax", 7, 0.8),
                                              ("odd-tied-sn", 4, 0.5), ("odd-vtable-sn", 5, 0.7)])
def test_generate_truncated_matches_oracle(name, top_k, top_p, fx):
    f = fx(name)
    model = load_model(f["root"])
    V = model.dev.V
    R, N = (12, 10) if name.startswith("peaked") else (40, 12)
    prompts = ragged_prompts(R, V, seed=len(name))
    ids, nll = model.generate(prompts, N, temperature=1.2, seed=77, top_k=top_k, top_p=top_p)
    assert len(ids) == R and all(len(x) == N and x.dtype == np.int64 for x in ids)
    agree, excused, onll = TR.oracle_follow(oracle_lm(f["root"]), prompts, ids, 1.2, 77, top_k, top_p, TOL_E2E)
    print("%s k %s p %s: %d draws agree, %d excused" % (name, top_k, top_p, agree, excused))
    assert excused <= max(1, (agree + excused) // 50), (agree, excused)
    for r in range(R):
        np.testing.assert_allclose(nll[r], onll[r], rtol=0, atol=TOK_ATOL, err_msg="%s row %d" % (name, r))
    # the nll is the full distribution's: score() of the generated sequences gives the same numbers
    sc = model.score([p[1:] + list(x) for p, x in zip(prompts, ids)], prompts[0][0])
    for r in range(R):
        np.testing.assert_allclose(nll[r], sc[r][-N:], rtol=0, atol=TOK_ATOL, err_msg="%s row %d (score)" % (name, r))
    # the truncation did something: the untruncated call draws other words somewhere
    plain, _ = model.generate(prompts, N, temperature=1.2, seed=77)
    assert any(not np.array_equal(a, b) for a, b in zip(ids, plain))


def test_generate_truncated_greedy_and_top1(fx):
    f = fx("small-vtable")
    model = load_model(f["root"])
    prompts = ragged_prompts(10, model.dev.V, seed=3)
    greedy, gn = model.generate(prompts, 8, temperature=0.0, seed=5)
    for kw in (dict(temperature=0.0, top_k=4, top_p=0.3), dict(temperature=0.7, top_k=1), dict(temperature=2.0, top_k=1, top_p=0.9)):
        ids, nll = model.generate(prompts, 8, seed=5, **kw)
        for a, b, c, d in zip(ids, greedy, nll, gn):
            assert np.array_equal(a, b), kw
            np.testing.assert_allclose(c, d, rtol=0, atol=1e-9)


@pytest.mark.parametrize("name", ["small-vtable", "small-char"])
def test_generate_truncated_cut_mixed_and_repeat(name, fx):
    f = fx(name)
    model = load_model(f["root"])
    prompts = ragged_prompts(37, model.dev.V, seed=11, lo=1, hi=9)
    kw = dict(temperature=0.8, seed=2 ** 64 - 3, top_k=6, top_p=0.85)
    ids, nll = model.generate(prompts, 9, **kw)
    ids2, nll2 = model.generate(prompts, 9, **kw)        # bit-identical run to run
    for a, b, c, d in zip(ids, ids2, nll, nll2):
        assert np.array_equal(a, b) and np.array_equal(c, d)
    for max_rows in (5, 13, 36):                         # the same rows cut three ways: the same draws
        ids3, nll3 = model.generate(prompts, 9, max_rows=max_rows, **kw)
        for r in range(37):
            assert np.array_equal(ids[r], ids3[r]), (max_rows, r)
            np.testing.assert_allclose(nll[r], nll3[r], rtol=0, atol=1e-9)
    for r in (0, 5, 36):                                 # a prompt among others = the same prompt alone, at the same row index
        solo, solo_nll = model.generate([prompts[r]] * (r + 1), 9, **kw)
        assert np.array_equal(solo[r], ids[r]), r
        np.testing.assert_allclose(solo_nll[r], nll[r], rtol=0, atol=1e-9)


def test_generate_truncated_odd_vocabulary_row_counts(fx):
    """V = 2 003: calls of 1, 31, 32 and 33 rows draw what the same rows draw inside a call of 64 (a row's u depends on its index alone)"""
    f = fx("odd-vtable")
    model = load_model(f["root"])
    assert model.dev.V == 2003
    prompts = ragged_prompts(64, 2003, seed=31, lo=1, hi=7)
    kw = dict(temperature=0.8, seed=123, top_k=6, top_p=0.85)
    ids, nll = model.generate(prompts, 9, **kw)
    for n in (1, 31, 32, 33):
        got, got_nll = model.generate(prompts[:n], 9, **kw)
        assert len(got) == n
        for r in range(n):
            assert np.array_equal(got[r], ids[r]), (n, r)
            np.testing.assert_allclose(got_nll[r], nll[r], rtol=0, atol=1e-9)


def test_generate_truncated_stop_id(fx):
    f = fx("small-vtable")
    model = load_model(f["root"])
    prompts = ragged_prompts(64, model.dev.V, seed=12)
    kw = dict(temperature=1.5, seed=9, top_k=12)
    full, full_nll = model.generate(prompts, 20, **kw)
    stop = int(np.argmax(np.bincount(np.concatenate(full), minlength=model.dev.V)))
    cut, cut_nll = model.generate(prompts, 20, stop_id=stop, **kw)
    n_stopped = 0
    for r in range(64):
        want = G.truncate(full[r], stop)
        assert np.array_equal(cut[r], want), r
        np.testing.assert_allclose(cut_nll[r], full_nll[r][:len(want)], rtol=0, atol=1e-9)
        n_stopped += len(want) < 20
    assert n_stopped >= 1


def test_generate_truncated_argument_errors(fx):
    model = load_model(fx("small-tied")["root"])
    for kw in (dict(top_k=0), dict(top_k=True), dict(top_k=2.5), dict(top_p=0.0), dict(top_p=1.01), dict(top_p=float("nan"))):
        with pytest.raises(ValueError):
            model.generate([[1]], 3, **kw)
    V = model.dev.V
    a, _ = model.generate([[1]] * 4, 5, seed=1)
    b, _ = model.generate([[1]] * 4, 5, seed=1, top_k=V, top_p=1.0)
    assert all(np.array_equal(x, z) for x, z in zip(a, b))


def test_first_word_frequencies_top_k_g_test(fx):
    """65 536 rows from <eos> with top_k = k*: no draw outside the oracle's k* best, and the first draws' frequencies against the
    oracle's renormalised head (G-test, bins with an expectation under 5 pooled).  k* in [4, 16] is the rank with the largest logit
    gap to the next, so the device and the oracle cannot disagree on the set."""
    f = fx("peaked20-vtable")
    model = load_model(f["root"])
    V = model.dev.V
    lm = oracle_lm(f["root"])
    h, c = lm.zero_state(1)
    h, c = lm.lstm_cell(np.array([G.EOS_ID]), h, c)
    y = lm.project(h)[0]
    order = TR.rank_order(y)
    gaps = y[order[3:16]] - y[order[4:17]]               # gap below rank k, k = 4 .. 16
    k_star = 4 + int(np.argmax(gaps))
    assert gaps.max() > TOL_E2E, gaps
    R = 65536
    ids, _nll = model.generate([[G.EOS_ID]] * R, 1, temperature=1.0, seed=2024, top_k=k_star)
    obs = np.bincount(np.array([x[0] for x in ids]), minlength=V).astype(np.float64)
    head = order[:k_star]
    assert obs.sum() == R and obs[head].sum() == R       # zero draws outside the kept set
    p = np.exp(y[head] - lse(y[head]))
    exp = p * R
    big = exp >= 5
    O = np.append(obs[head][big], obs[head][~big].sum())
    E = np.append(exp[big], exp[~big].sum())
    keep = E > 0
    O, E = O[keep], E[keep]
    nz = O > 0
    g = 2.0 * float((O[nz] * np.log(O[nz] / E[nz])).sum())
    k = len(O) - 1
    assert k >= 2, k
    pval = _chi2_sf_wh(g, k)
    print("k* %d, G %.3f on %d degrees of freedom, p-value %.4g" % (k_star, g, k, pval))
    assert pval > 1e-4, (g, k, pval)


def test_generate_truncated_cli(fx, capsys):
    from jlm_amd import generate as gen_mod
    f = fx("small-vtable")
    ids, nll = gen_mod.main(["--root", f["root"], "-e", "1", "-n", "5", "--words", "7", "--seed", "3", "--top-k", "5", "--top-p", "0.8",
                             "--show-nll"])
    out = _samples(capsys)
    assert len(out) == 5 and len(ids) == 5
    for line, x, l in zip(out, ids, nll):
        _text, tot, n = line.split("\t")
        assert int(n) == len(x) == 7
        assert abs(float(tot) - l.sum()) < 1e-3
    model = load_model(f["root"])
    want, _ = model.generate([[G.EOS_ID]] * 5, 7, seed=3, top_k=5, top_p=0.8)
    assert all(np.array_equal(a, b) for a, b in zip(ids, want))
