"""GPU: batched ancestral sampling (LSTM_Model.generate, python -m jlm_amd.generate; csrc jlm_generate_frames + sample_rows_kernel).

Kernel level (torch.ops.jlm.sample_rows over logits the test writes): the draws equal a float64 inverse CDF over the same f32 logits
with the same u, except where u S lies within a relative 1e-9 of a boundary (counted, and asserted rare); greedy draws are the argmax
with the lowest id winning a tie; the nll is within 1e-6 of the float64 lse - y.

End to end, against the oracle's OracleLM (oracle/jlm_oracle.py, float64) teacher-forced on the device's draws: every draw whose u is
not within TOL_E2E of a boundary of the oracle's CDF is the oracle's draw; nll within 1e-5 per token of the oracle and of score()."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
from jlm_amd import _lib, generate as G, ops as _ops                                     # noqa: E402
from tests.gpu_rows import UNTIED_F32, fixture_model, load_model, lse, oracle_lm, ragged_prompts     # noqa: E402

pytestmark = pytest.mark.gpu

TOK_ATOL = 1e-5
TOL_E2E = 1e-4          # the device's logits differ from float64 ones by ~1e-6: a CDF boundary this close is ambiguous


def _dev():
    return _lib.require_gpu()


def _sample(y, temperature, seed, step, row_id=None, forced=None, done=None, stop_id=-1, self_norm=False, n_dev=None, word0=None):
    """one jlm_sample_rows launch over y [R, n_cols] (f32 numpy) -> (ids, nll, word, flags, done)"""
    dev = _dev()
    R, n = y.shape
    ld = (n + 3) // 4 * 4
    yp = np.full((R, ld), np.nan, dtype=np.float32)        # the padding is never read as a word
    yp[:, :n] = y
    yt = torch.from_numpy(yp).to(dev)
    it = lambda a: None if a is None else torch.as_tensor(np.asarray(a, dtype=np.int32)).to(dev)
    word = it(np.zeros(R) if word0 is None else word0)
    ids = torch.full((R,), -7, device=dev, dtype=torch.int32)
    nll = torch.zeros(R, device=dev, dtype=torch.float64)
    flags = torch.zeros(1, device=dev, dtype=torch.int32)
    dn = it(done)
    _ops.backend().sample_rows(yt, ld, n, R, it(n_dev), float(temperature), int(seed), int(step), it(row_id), it(forced), dn,
                               int(stop_id), bool(self_norm), word, ids, nll, flags)
    torch.cuda.synchronize()
    return (ids.cpu().numpy(), nll.cpu().numpy(), word.cpu().numpy(), int(flags.cpu()[0]),
            None if dn is None else dn.cpu().numpy())


def _masses(y, temperature):
    """float64 masses of f32 logits: the tempered argument formed in f32 as the kernel forms it, exp in float64"""
    y = np.asarray(y, dtype=np.float32)
    m = y.max()
    x = (y - m) * np.float32(1.0 / temperature)
    return np.exp(x.astype(np.float64))


def _check_draw(y, temperature, u, got, tol):
    """-> True when `got` is the float64 inverse-CDF draw, False when it differs but u S lies within a relative `tol` of its
    interval's ends (ambiguous); asserts otherwise"""
    mass = _masses(y, temperature)
    want = G.inverse_cdf(mass, u)
    if got == want:
        return True
    c = np.cumsum(mass)
    S, t = c[-1], u * c[-1]
    lo = c[got - 1] if got > 0 else 0.0
    hi = c[got]
    assert 0 <= got < len(y) and mass[got] > 0, (got, want)
    assert lo - tol * S <= t <= hi + tol * S, ("draw %d outside its CDF interval" % got, want, t / S, lo / S, hi / S)
    return False


def _kernel_case(y, temperature, seed=5, steps=3, self_norm=False):
    R, n = y.shape
    ambiguous = total = 0
    row_id = np.arange(R) * 3 + 11
    for step in range(steps):
        ids, nll, word, fl, _ = _sample(y, temperature, seed, step, row_id=row_id, self_norm=self_norm)
        assert fl == 0
        assert np.array_equal(ids, word)
        u = G.uniform(seed, step, row_id)
        for r in range(R):
            if temperature == 0:
                assert ids[r] == int(np.argmax(y[r]))
            else:
                ambiguous += not _check_draw(y[r], temperature, u[r], int(ids[r]), 1e-9)
            want = -float(y[r, ids[r]]) if self_norm else lse(y[r]) - float(y[r, ids[r]])
            assert abs(nll[r] - want) <= 1e-6, (r, nll[r], want)
            total += 1
    assert ambiguous <= max(1, total // 100), (ambiguous, total)
    return total


@pytest.mark.parametrize("n_cols", [1, 63, 64, 1025, 50000, 100003])
@pytest.mark.parametrize("temperature", [0.05, 1.0, 10.0])
def test_sample_rows_random_logits(n_cols, temperature):
    rng = np.random.RandomState(n_cols)
    R = 96 if n_cols <= 1025 else 24
    y = (rng.standard_normal((R, n_cols)) * 3).astype(np.float32)
    _kernel_case(y, temperature)


@pytest.mark.parametrize("temperature", [0.05, 1.0, 10.0])
def test_sample_rows_special_rows(temperature):
    rng = np.random.RandomState(4)
    n = 5003
    eq = np.full((8, n), 1.25, dtype=np.float32)                          # equal logits: a uniform draw
    dom = (rng.standard_normal((8, n))).astype(np.float32)
    dom[np.arange(8), rng.randint(0, n, size=8)] = 40.0                   # one dominant word
    pm = rng.choice([-30.0, 30.0], size=(8, n)).astype(np.float32)        # logits of +-30
    for y in (eq, dom, pm):
        _kernel_case(y, temperature)
    ids, _nll, _w, fl, _ = _sample(eq, temperature, 1, 0)
    u = G.uniform(1, 0, np.arange(8))
    assert np.array_equal(ids, np.minimum((u * n).astype(np.int64), n - 1))   # equal masses: floor(u n)


def test_sample_rows_self_norm():
    y = (np.random.RandomState(8).standard_normal((32, 777)) * 2).astype(np.float32)
    _kernel_case(y, 1.0, self_norm=True)
    _kernel_case(y, 0.0, self_norm=True)


def test_sample_rows_greedy_ties():
    rng = np.random.RandomState(6)
    n = 3000
    y = rng.standard_normal((16, n)).astype(np.float32)
    for r in range(16):                      # the maximum at 2-4 places; the lowest id must win
        pos = np.sort(rng.choice(n, size=2 + r % 3, replace=False))
        y[r, pos] = 9.0
    _kernel_case(y, 0.0, steps=1)
    ids, _nll, _w, _fl, _ = _sample(np.full((3, 1025), -2.0, dtype=np.float32), 0.0, 0, 0)
    assert ids.tolist() == [0, 0, 0]


def test_sample_rows_nan_sets_flag():
    y = np.random.RandomState(2).standard_normal((4, 2000)).astype(np.float32)
    y[2, 777] = np.nan
    ids, _nll, word, fl, _ = _sample(y, 1.0, 0, 0)
    assert fl & 1
    assert ids[2] == -1 and 0 <= word[2] < 2000
    y[2, 777] = np.inf
    assert _sample(y, 1.0, 0, 0)[3] & 1


def test_sample_rows_forced_done_and_live_count():
    rng = np.random.RandomState(9)
    y = rng.standard_normal((6, 300)).astype(np.float32)
    forced = [-1, 17, -1, -1, -1, -1]
    done = [0, 0, 1, 0, 0, 0]
    ids, nll, word, fl, dn = _sample(y, 1.0, 3, 2, forced=forced, done=done, stop_id=-1, n_dev=[5], word0=[9] * 6)
    assert fl == 0
    assert word[1] == 17 and ids[1] == -1                # forced: passes through
    assert ids[2] == -1 and word[2] == 9 and dn[2] == 1  # stopped: masked, its word kept
    assert ids[5] == -7 and word[5] == 9                 # past the live count: untouched
    for r in (0, 3, 4):
        assert ids[r] == word[r] >= 0
    # a draw of the stop word marks the row done
    ids2, _n, _w, _f, dn2 = _sample(y, 1.0, 3, 2, done=[0] * 6, stop_id=int(ids[0]))
    assert dn2[0] == 1 and ids2[0] == ids[0]


# ------------------------------------------------------------------------------------------------------------- end to end
SMALL = ["small-tied", "small-untied", "small-dsoftmax", "small-vtable", "small-tied-sn", "small-vtable-sn",
         "wide-vtable", "wide-dsoftmax", "wideh-vtable", "wide128-tied", "small-char"]


def oracle_follow(lm, prompts, ids, temperature, seed, n_words):
    """the oracle teacher-forced on the device's draws: -> (agreeing draws, ambiguous draws, oracle nll per row)"""
    sn = lm.config["self_norm"]
    agree = amb = 0
    out = []
    for r, (p, x) in enumerate(zip(prompts, ids)):
        h, c = lm.zero_state(1)
        for w in p:
            h, c = lm.lstm_cell(np.array([w]), h, c)
        nll = []
        for k, w in enumerate(x):
            y = lm.project(h)[0]
            nll.append(-y[w] if sn else lse(y) - y[w])
            if temperature == 0:
                srt = np.sort(y)
                if w == int(np.argmax(y)):
                    agree += 1
                else:
                    assert srt[-1] - y[w] <= TOL_E2E, (r, k, w, int(np.argmax(y)))
                    amb += 1
            else:
                mass = np.exp((y - y.max()) / temperature)
                u = float(G.uniform(seed, k, r))
                want = G.inverse_cdf(mass, u)
                if want == w:
                    agree += 1
                else:
                    cdf = np.cumsum(mass)
                    S, t = cdf[-1], u * cdf[-1]
                    lo = cdf[w - 1] if w > 0 else 0.0
                    assert lo - TOL_E2E * S <= t <= cdf[w] + TOL_E2E * S, (r, k, w, want, t / S)
                    amb += 1
            h, c = lm.lstm_cell(np.array([w]), h, c)
        out.append(np.array(nll))
    return agree, amb, out


# V = 2 003 cut at 501 / 1 203 (jlm_amd/synth.py): ld_logits > V, every segment's logits start at an unaligned column
ODD = ["odd-tied", "odd-untied", "odd-dsoftmax", "odd-vtable", "odd-tied-sn", "odd-vtable-sn", "oddw-vtable", "odd-untied@f32"]


@pytest.mark.parametrize("name", SMALL + ["peaked20-vtable", UNTIED_F32] + ODD)
def test_generate_matches_oracle(name, fx, monkeypatch):
    f, model = fixture_model(fx, name, monkeypatch)
    V = model.dev.V
    R, N = (12, 10) if name.startswith("peaked") else (40, 12)
    prompts = ragged_prompts(R, V, seed=len(name))
    ids, nll = model.generate(prompts, N, temperature=1.0, seed=77)
    assert len(ids) == R and all(len(x) == N and x.dtype == np.int64 for x in ids)
    assert all(l.dtype == np.float64 for l in nll)
    agree, amb, onll = oracle_follow(oracle_lm(f["root"]), prompts, ids, 1.0, 77, N)
    assert amb <= max(1, (agree + amb) // 50), (agree, amb)
    for r in range(R):
        np.testing.assert_allclose(nll[r], onll[r], rtol=0, atol=TOK_ATOL, err_msg="%s row %d" % (name, r))
    # score() of the generated sequences: the same -log p on the generated positions
    sc = model.score([p[1:] + list(x) for p, x in zip(prompts, ids)], prompts[0][0])
    for r in range(R):
        np.testing.assert_allclose(nll[r], sc[r][-N:], rtol=0, atol=TOK_ATOL, err_msg="%s row %d (score)" % (name, r))


@pytest.mark.parametrize("name,temperature", [("small-vtable", 0.0), ("small-tied-sn", 0.0), ("peaked20-vtable", 0.0),
                                              ("small-dsoftmax", 0.05), ("small-untied", 10.0)])
def test_generate_temperatures_against_oracle(name, temperature, fx):
    f = fx(name)
    model = load_model(f["root"])
    prompts = ragged_prompts(10, model.dev.V, seed=3)
    ids, nll = model.generate(prompts, 8, temperature=temperature, seed=5)
    agree, amb, onll = oracle_follow(oracle_lm(f["root"]), prompts, ids, temperature, 5, 8)
    assert amb <= 1, (agree, amb)
    for r in range(len(prompts)):
        np.testing.assert_allclose(nll[r], onll[r], rtol=0, atol=TOK_ATOL)


@pytest.mark.parametrize("name", ["small-vtable", "small-char", "wide-vtable"])
def test_generate_cut_mixed_and_repeat(name, fx):
    f = fx(name)
    model = load_model(f["root"])
    V = model.dev.V
    prompts = ragged_prompts(37, V, seed=11, lo=1, hi=9)
    ids, nll = model.generate(prompts, 9, temperature=0.8, seed=2 ** 64 - 3)
    # bit-identical run to run
    ids2, nll2 = model.generate(prompts, 9, temperature=0.8, seed=2 ** 64 - 3)
    for a, b, c, d in zip(ids, ids2, nll, nll2):
        assert np.array_equal(a, b) and np.array_equal(c, d)
    # the same rows cut into calls of 5: same draws
    ids3, nll3 = model.generate(prompts, 9, temperature=0.8, seed=2 ** 64 - 3, max_rows=5)
    for r in range(37):
        assert np.array_equal(ids[r], ids3[r]), r
        np.testing.assert_allclose(nll[r], nll3[r], rtol=0, atol=1e-9)
    # a prompt among prompts of other lengths = the same prompt in a call of that prompt alone (at the same row index)
    for r in (0, 5, 36):
        solo, solo_nll = model.generate([prompts[r]] * (r + 1), 9, temperature=0.8, seed=2 ** 64 - 3)
        assert np.array_equal(solo[r], ids[r]), r
        np.testing.assert_allclose(solo_nll[r], nll[r], rtol=0, atol=1e-9)


def test_generate_odd_vocabulary_row_counts(fx):
    """V = 2 003: calls of 1, 31, 32 and 33 rows draw what the same rows draw inside a call of 64 (a row's u depends on its index alone)"""
    f = fx("odd-vtable")
    model = load_model(f["root"])
    assert model.dev.V == 2003
    prompts = ragged_prompts(64, 2003, seed=31, lo=1, hi=7)
    ids, nll = model.generate(prompts, 9, temperature=0.8, seed=123)
    for n in (1, 31, 32, 33):
        got, got_nll = model.generate(prompts[:n], 9, temperature=0.8, seed=123)
        assert len(got) == n
        for r in range(n):
            assert np.array_equal(got[r], ids[r]), (n, r)
            np.testing.assert_allclose(got_nll[r], nll[r], rtol=0, atol=1e-9)


def test_generate_stop_id(fx):
    f = fx("small-vtable")
    model = load_model(f["root"])
    prompts = ragged_prompts(64, model.dev.V, seed=12)
    full, full_nll = model.generate(prompts, 20, temperature=1.5, seed=9)
    counts = np.bincount(np.concatenate(full), minlength=model.dev.V)
    stop = int(np.argmax(counts))
    cut, cut_nll = model.generate(prompts, 20, temperature=1.5, seed=9, stop_id=stop)
    n_stopped = 0
    for r in range(64):
        want = G.truncate(full[r], stop)
        assert np.array_equal(cut[r], want), r
        np.testing.assert_allclose(cut_nll[r], full_nll[r][:len(want)], rtol=0, atol=1e-9)
        n_stopped += len(want) < 20
    assert n_stopped >= 1


def test_generate_default_prompt_and_errors(fx):
    f = fx("small-tied")
    model = load_model(f["root"])
    ids, nll = model.generate(None, 5, seed=1)
    assert len(ids) == 1 and len(ids[0]) == 5
    one, _ = model.generate([[G.EOS_ID]], 5, seed=1)
    assert np.array_equal(one[0], ids[0])
    assert [len(x) for x in model.generate([[1], [2, 3]], 0)[0]] == [0, 0]
    V = model.dev.V
    for kw in (dict(prompts=[[V]]), dict(prompts=[[]]), dict(n_words=-1), dict(temperature=-1.0), dict(temperature=float("nan"))):
        args = dict(prompts=[[1]], n_words=3)
        args.update(kw)
        with pytest.raises(ValueError):
            model.generate(**args)


def _chi2_sf_wh(x, k):
    """upper tail of chi^2_k (Wilson-Hilferty)"""
    from math import erfc, sqrt
    z = ((x / k) ** (1.0 / 3) - (1 - 2.0 / (9 * k))) / sqrt(2.0 / (9 * k))
    return 0.5 * erfc(z / sqrt(2.0))


def test_first_word_frequencies_g_test(fx):
    """65 536 rows from <eos>: the first draws' frequencies against the oracle's distribution (G-test, bins with an expectation
    under 5 pooled)"""
    f = fx("peaked20-vtable")
    model = load_model(f["root"])
    V = model.dev.V
    R = 65536
    ids, _nll = model.generate([[G.EOS_ID]] * R, 1, temperature=1.0, seed=2024)
    obs = np.bincount(np.array([x[0] for x in ids]), minlength=V).astype(np.float64)
    lm = oracle_lm(f["root"])
    h, c = lm.zero_state(1)
    h, c = lm.lstm_cell(np.array([G.EOS_ID]), h, c)
    y = lm.project(h)[0]
    p = np.exp(y - lse(y))
    exp = p * R
    big = exp >= 5
    O = np.append(obs[big], obs[~big].sum())
    E = np.append(exp[big], exp[~big].sum())
    keep = E > 0
    O, E = O[keep], E[keep]
    nz = O > 0
    g = 2.0 * float((O[nz] * np.log(O[nz] / E[nz])).sum())
    k = len(O) - 1
    assert k >= 5, k                         # a peaked model, but several words in play
    pval = _chi2_sf_wh(g, k)
    assert pval > 1e-4, (g, k, pval)


def _samples(capsys):
    """the CLI's sample lines (the model loader announces itself on stdout first)"""
    return [l for l in capsys.readouterr().out.strip().split("\n") if not l.startswith("LSTM model:")]


@pytest.mark.parametrize("name", ["small-vtable", "small-char"])
def test_generate_cli(name, fx, capsys):
    from jlm_amd import generate as gen_mod
    f = fx(name)
    ids, nll = gen_mod.main(["--root", f["root"], "-e", "1", "-n", "5", "--words", "7", "--temperature", "0.9", "--seed", "3",
                             "--show-nll"])
    out = _samples(capsys)
    assert len(out) == 5 and len(ids) == 5
    for line, x, l in zip(out, ids, nll):
        text, tot, n = line.split("\t")
        assert int(n) == len(x) == 7
        assert abs(float(tot) - l.sum()) < 1e-3
    # a prompt from the lexicon, stopping at <eos>
    lex = f["lexicon"]
    prompt = " ".join(w for w, _c in lex[3:5])
    gen_mod.main(["--root", f["root"], "-e", "1", "-n", "3", "--words", "6", "--prompt", prompt, "--stop-at-eos"])
    out = _samples(capsys)
    assert len(out) == 3
    head = "".join(w.split("/")[0] for w, _c in lex[3:5]) if name == "small-char" else " ".join(w.split("/")[0] for w, _c in lex[3:5])
    assert all(line.startswith(head) for line in out)
