"""GPU: prediction from a typed reading prefix (LSTM_Model.predict_reading / complete_reading, predict_top(allowed=),
complete(first_allowed=), python -m jlm_amd.complete --reading; csrc topk_rows_masked_kernel + jlm_complete_frames_masked).

Kernel level: torch.ops.jlm.topk_rows_masked over logits the test writes gives exactly the ids of complete.topk_masked_reference (a
numpy ranking of the allowed words, padded with -1 / +inf), nll within 1e-6 of the f64 lse over the WHOLE row minus y (-y exactly on
self-normalised rows; tests/test_gpu_complete.py's bars for the same arithmetic); rows of set -1 equal torch.ops.jlm.topk_rows bit for
bit; torch.ops.jlm.beam_merge fed the kernel's own padded lists equals complete.merge_reference bit for bit.

End to end, against the oracle's OracleLM (float64): predict_reading returns the oracle's best allowed words, complete_reading follows
test_gpu_complete.oracle_follow's rule with frame 0 restricted to the set, under that file's bars (TOL_E2E, TOK_ATOL, the share of
ambiguous frames)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
from jlm_amd import complete as C, ops as _ops, synth                                     # noqa: E402
from jlm_amd.readings import ReadingIndex, reading_of                                     # noqa: E402
from tests.gpu_rows import UNTIED_F32, fixture_model, load_model, lse, oracle_lm, ragged_prompts     # noqa: E402
from tests.test_gpu_complete import TOK_ATOL, TOL_E2E, _dev, _lines, _merge, _topk                  # noqa: E402

pytestmark = pytest.mark.gpu

KANA = synth.KANA


def _topk_masked(y, k, sets, self_norm=False, ld_mask=None, row_set=None, n_sets=None):
    """one jlm_topk_rows_masked launch over y [R, n_cols] (f32 numpy); sets: per row None (set -1) or word ids
    -> (ids [R, k], nll [R, k], flags)"""
    dev = _dev()
    R, n = y.shape
    ld = (n + 3) // 4 * 4
    yp = np.full((R, ld), np.nan, dtype=np.float32)        # the padding is never read as a word
    yp[:, :n] = y
    restricted = [r for r in range(R) if sets[r] is not None]
    mask, which = ReadingIndex.mask([sets[r] for r in restricted], n)
    rs = [-1] * R
    for r, s in zip(restricted, which):
        rs[r] = int(s)
    if ld_mask is not None:
        mask = np.ascontiguousarray(mask[:, :ld_mask])
    ids = torch.full((R, k), -7, device=dev, dtype=torch.int32)
    nll = torch.zeros((R, k), device=dev, dtype=torch.float64)
    flags = torch.zeros(1, device=dev, dtype=torch.int32)
    _ops.backend().topk_rows_masked(torch.from_numpy(yp).to(dev), ld, n, R, k, bool(self_norm),
                                    torch.from_numpy(mask.view(np.int32)).to(dev), mask.shape[1],
                                    mask.shape[0] if n_sets is None else n_sets, rs if row_set is None else row_set, ids, nll, k, flags)
    torch.cuda.synchronize()
    return ids.cpu().numpy(), nll.cpu().numpy(), int(flags.cpu()[0])


def _check_masked(y, k, sets, flagged=()):
    """both forms of the kernel over y with the rows' sets against the restatement; rows of set None against jlm_topk_rows"""
    for sn in (False, True):
        ids, nll, fl = _topk_masked(y, k, sets, sn)
        assert (fl & 1) == (1 if flagged else 0)
        plain = None
        for r in range(y.shape[0]):
            if r in flagged:
                assert np.all(ids[r] == -1) and np.all(np.isnan(nll[r])), r
                continue
            if sets[r] is None:
                if plain is None:
                    keep = [q for q in range(y.shape[0]) if sets[q] is None and q not in flagged]
                    plain = dict(zip(keep, zip(*_topk(y[keep], k, sn)[:2])))
                assert np.array_equal(ids[r], plain[r][0]) and np.array_equal(nll[r], plain[r][1]), r     # bit for bit
                continue
            want_ids, want_nll = C.topk_masked_reference(y[r], k, sets[r], sn)
            assert ids[r].tolist() == want_ids.tolist(), (r, sn, ids[r][:8], want_ids[:8])
            pad = want_ids < 0
            assert np.all(np.isposinf(nll[r][pad]))
            if sn:
                assert np.array_equal(nll[r], want_nll)
            else:
                inf = np.isinf(want_nll)                                     # the padding, or an allowed word at -inf
                assert np.array_equal(np.isposinf(nll[r]), inf)
                np.testing.assert_allclose(nll[r][~inf], want_nll[~inf], rtol=0, atol=1e-6)
    return ids, nll


def _wave_span(n_cols, wave):
    """the word ids of one wave's span in topk_rows_kernel's layout (4 waves, 64 lanes x 4 words an iteration)"""
    n_it = ((n_cols + 3) // 4 + 63) // 64
    ipw = (n_it + 3) // 4
    return np.arange(min(wave * ipw * 256, n_cols), min((wave + 1) * ipw * 256, n_cols))


SHAPES = [(n, k) for n in (1, 63, 64, 65, 1000, 5003, 50000) for k in (1, 10, 64) if k <= n]


@pytest.mark.parametrize("n_cols,k", SHAPES)
def test_topk_rows_masked_random_logits(n_cols, k):
    rng = np.random.RandomState(n_cols * 100 + k)
    n = n_cols
    pick = lambda m: np.sort(rng.choice(n, size=min(max(m, 0), n), replace=False))
    span = next(s for s in (_wave_span(n, w) for w in (3, 2, 1, 0)) if len(s))
    sets = [np.array([], dtype=np.int64),                                    # empty: all padding
            pick(1), pick(k - 1), pick(k), pick(k + 1),
            np.arange(n),                                                    # every word
            np.arange(4 * ((n - 1) // 4), n),                                # only words of the last (partial) 4-word chunk
            span[rng.rand(len(span)) < 0.5] if len(span) > 1 else span,      # only words inside one wave's span
            None,                                                            # (the complement of the row's top k: below)
            np.flatnonzero(rng.rand(n) < 0.5),                               # a random half
            None, None]                                                      # unrestricted rows in the same launch
    R = len(sets)
    y = (rng.standard_normal((R, n)) * 3).astype(np.float32)
    top = C.topk_reference(y[8], k)[0]
    sets[8] = np.setdiff1d(np.arange(n), top)                                # the row's maximum is not allowed
    assert R <= 24 and (n == k or int(np.argmax(y[8])) not in sets[8])
    ids, _nll = _check_masked(y, k, sets)
    assert np.all(ids[0] == -1)


@pytest.mark.parametrize("k", [1, 10, 64])
def test_topk_rows_masked_special_rows(k):
    rng = np.random.RandomState(k)
    n = 5003
    half = lambda: np.flatnonzero(rng.rand(n) < 0.5)
    rows = [np.full(n, 1.25, dtype=np.float32),                              # all equal: the k lowest allowed ids
            np.arange(n, dtype=np.float32) * 1e-3,                           # ascending: ~625 appends a wave, past TK_CAP = 512
            -np.arange(n, dtype=np.float32) * 1e-3,                          # descending
            rng.randint(-2, 3, size=n).astype(np.float32)]                   # five values: ties everywhere
    sets = [half() for _ in rows]
    straddle = rng.standard_normal(n).astype(np.float32)
    allowed = half()
    top = np.sort(rng.choice(allowed, size=k + 5, replace=False))
    straddle[top[:k - 1]] = 8.0
    straddle[top[k - 1:]] = 7.0                                              # six equal allowed logits at the k-th place ...
    others = np.setdiff1d(np.arange(n), allowed)
    straddle[others[:7]] = 7.0                                               # ... and disallowed ones among them, and above
    straddle[others[7:9]] = 9.0
    rows.append(straddle)
    sets.append(allowed)
    rows.append(rows[1].copy())                                              # the ascending row again, unrestricted
    sets.append(None)
    y = np.stack(rows)
    ids, _nll = _check_masked(y, k, sets)
    assert ids[0].tolist() == sets[0][:k].tolist()
    assert ids[1].tolist() == sets[1][::-1][:k].tolist()
    assert ids[4].tolist() == top[:k].tolist()


def test_topk_rows_masked_non_finite():
    rng = np.random.RandomState(2)
    n, k = 2000, 10
    y = rng.standard_normal((5, n)).astype(np.float32)
    sets = [np.flatnonzero(rng.rand(n) < 0.5) for _ in range(4)] + [None]
    out = int(np.setdiff1d(np.arange(n), sets[2])[3])
    y[2, out] = np.nan                                                       # a NaN at a DISALLOWED word still flags the row
    ids, nll, fl = _topk_masked(y, k, sets)
    assert fl & 1 and np.all(ids[2] == -1) and np.all(np.isnan(nll[2]))
    for r in (0, 1, 3):
        assert ids[r].tolist() == C.topk_masked_reference(y[r], k, sets[r])[0].tolist()
    y[2, out] = np.inf
    assert _topk_masked(y, k, sets)[2] & 1
    assert _topk_masked(y, k, sets, self_norm=True)[2] & 1
    y[2, out] = -np.inf                                                      # a -inf logit is a word of probability 0: no flag
    assert _topk_masked(y, k, sets)[2] == 0
    # an ALLOWED word at -inf ranks (last) and is no flag; the padding follows it
    a, b = int(sets[1][0]), int(sets[1][5])
    y[1, b] = -np.inf
    small = list(sets)
    small[1] = np.array([b, a])
    ids, nll, fl = _topk_masked(y, 3, small)
    assert fl == 0 and ids[1].tolist() == [a, b, -1] and np.isfinite(nll[1, 0]) and np.all(np.isposinf(nll[1, 1:]))
    _check_masked(y, 3, small)


def test_topk_rows_masked_refuses_bad_sets():
    y = np.random.RandomState(3).standard_normal((3, 100)).astype(np.float32)
    sets = [np.array([1, 2, 3]), None, np.array([50, 99])]
    bad = [dict(row_set=[0, -1, 2]), dict(row_set=[0, -2, 1]), dict(row_set=[0, -1]), dict(row_set=[0, -1, 1, 1]),
           dict(ld_mask=3), dict(n_sets=3), dict(n_sets=-1), dict(n_sets=1)]       # ceil(100 / 32) = 4 words a set; 2 sets
    for kw in bad:
        with pytest.raises(RuntimeError):
            _topk_masked(y, 5, sets, **kw)
    dev = _dev()
    ids = torch.full((3, 5), -7, device=dev, dtype=torch.int32)                  # ... and nothing is launched
    nll = torch.zeros((3, 5), device=dev, dtype=torch.float64)
    mask = torch.zeros((2, 4), device=dev, dtype=torch.int32)
    with pytest.raises(RuntimeError):
        _ops.backend().topk_rows_masked(torch.zeros((3, 100), device=dev), 100, 100, 3, 5, False, mask, 4, 2, [0, 2, 1], ids, nll, 5, None)
    torch.cuda.synchronize()
    assert np.all(ids.cpu().numpy() == -7)
    assert _topk_masked(y, 5, sets)[2] == 0


@pytest.mark.parametrize("B", [1, 6, 64])
def test_beam_merge_on_padded_lists(B):
    rng = np.random.RandomState(B)
    NP, V = 6, 300
    R = NP * B
    y = (rng.randint(-6, 7, size=(R, V)) * 0.5).astype(np.float32)          # a coarse grid: equal nll and equal scores
    sizes = [0, 1, max(B - 1, 1), B, B + 3]
    sets = [np.sort(rng.choice(V, size=s, replace=False)) for s in sizes] + [None]
    ci0, cn0, fl = _topk_masked(y[:NP], B, sets)
    assert fl == 0 and np.all(ci0[0] == -1) and (B == 1 or ci0[1, 1] == -1)
    ci, cn, fl = _topk(y, B)                                                 # a following frame's lists: every row unrestricted
    assert fl == 0
    for stop_id in (-1, int(ci0[3, 0])):
        got = _merge(np.concatenate([ci0, ci[NP:]]), np.concatenate([cn0, cn[NP:]]), np.zeros(R), np.zeros(R, np.int32), B, NP, True, stop_id)
        want = C.merge_reference(ci0, cn0, None, None, B, NP, True, stop_id)
        for key in ("bp_parent", "bp_word", "score", "finished", "prev", "word", "bp_nll"):
            assert np.array_equal(got[key], want[key]), (key, stop_id)
        assert np.all(got["finished"][:B] == 1) and np.all(np.isposinf(got["score"][:B]))            # the empty set: all padding
        # the following frame: the padding's hypotheses are dead parents -- carried, never expanded, behind every finite candidate
        got2 = _merge(ci, cn, got["score"], got["finished"], B, NP, False, stop_id)
        want2 = C.merge_reference(ci, cn, want["score"], want["finished"], B, NP, False, stop_id)
        for key in ("bp_parent", "bp_word", "score", "finished", "prev", "word", "bp_nll"):
            assert np.array_equal(got2[key], want2[key]), (key, stop_id)
        for p in range(1, NP):
            live = int((got["finished"][p * B:(p + 1) * B] == 0).sum())
            if live:                                                        # one live parent's B candidates already fill the beam
                assert np.all(np.isfinite(got2["score"][p * B:(p + 1) * B])), p


# ------------------------------------------------------------------------------------------------------------- end to end
def _prefixes(n):
    one = [KANA[p % 12] for p in range(n)]
    two = [KANA[p % 12] + KANA[(p * 5 + 1) % 12] for p in range(n)]
    return one, two


def _oracle_logp(lm, prompt):
    """-> (h, c, log p of every next word after the prompt), float64"""
    h, c = lm.zero_state(1)
    for w in prompt:
        h, c = lm.lstm_cell(np.array([w]), h, c)
    y = lm.project(h)[0]
    return h, c, (y if lm.config["self_norm"] else y - lse(y))


def _follow(lm, prompt, allowed, bp_parent, bp_word, bp_nll, score, p, N, B):
    """test_gpu_complete.oracle_follow with frame 0's candidates restricted to ``allowed``; a set smaller than B leaves padding
    (word -1, score +inf, finished) in the device's first beam.  -> (agreeing frames, ambiguous frames)"""
    sn = lm.config["self_norm"]
    h, c = lm.zero_state(1)
    for w in prompt:
        h, c = lm.lstm_cell(np.array([w]), h, c)
    beam = [dict(h=h[0], c=c[0], s=0.0, fin=False, n=0)]
    agree = amb = 0
    for k in range(N):
        Y = lm.project(np.stack([b["h"] for b in beam]))
        cands = []
        for j, b in enumerate(beam):
            if b["fin"]:
                cands.append((b["s"], j, -1))
                continue
            y = Y[j]
            tot = b["s"] + (-y if sn else lse(y) - y)
            words = np.asarray(allowed) if k == 0 else np.arange(len(y))
            top = words[np.argsort(tot[words], kind="stable")[:B + 1]]
            cands.extend((float(tot[w]), j, int(w)) for w in top)
        cands.sort()
        q = p * B + np.arange(B)
        dev_set = set((j, w) for j, w in zip(bp_parent[k, q].tolist(), bp_word[k, q].tolist()) if w >= 0 or k > 0)    # (not the padding)
        if k == 0:
            assert sum(w < 0 for w in bp_word[0, q]) == max(0, B - len(allowed))     # padding only where the set runs out
        want_set = set((j, w) for _s, j, w in cands[:B])
        if dev_set == want_set:
            agree += 1
        else:
            gap = cands[B][0] - cands[B - 1][0] if len(cands) > B else 0.0
            assert gap < TOL_E2E, ("frame %d: kept set differs from the oracle's with a clear cut" % k, gap, dev_set ^ want_set)
            amb += 1
        nb = []
        for i in range(B):
            j, w, n = int(bp_parent[k, q[i]]), int(bp_word[k, q[i]]), float(bp_nll[k, q[i]])
            if w < 0 and k == 0:
                assert n == np.inf
                nb.append(dict(h=beam[0]["h"], c=beam[0]["c"], s=np.inf, fin=True, n=0))
                continue
            par = beam[j]
            if w < 0:
                assert par["fin"] and n == 0.0
                nb.append(dict(par))
                continue
            y = Y[j]
            on = -y[w] if sn else lse(y) - y[w]
            assert abs(n - on) <= TOK_ATOL, (k, i, n, on)
            h2, c2 = lm.lstm_cell(np.array([w]), par["h"][None], par["c"][None])
            nb.append(dict(h=h2[0], c=c2[0], s=par["s"] + on, fin=False, n=par["n"] + 1))
        beam = nb
    for i in range(B):
        got, want = score[p * B + i], beam[i]["s"]
        assert (got == want) if np.isinf(want) else abs(got - want) <= TOK_ATOL * max(1, beam[i]["n"]), (p, i, got, want)
    return agree, amb


def _e2e_reading(name, fx, monkeypatch, R):
    f, model = fixture_model(fx, name, monkeypatch)
    V = model.dev.V
    prompts = ragged_prompts(R, V, seed=len(name))
    lm = oracle_lm(f["root"])
    index = model.reading_index()
    oracle = [_oracle_logp(lm, p)[2] for p in prompts]
    start = prompts[0][0]
    for prefixes in _prefixes(R):
        sets = [index.lookup(x) for x in prefixes]
        for n in (6, 64):
            res = model.predict_reading(prompts, prefixes, n=n)
            seqs, lps = [], []
            for p, (ids, logp) in enumerate(res):
                a, lp = sets[p], oracle[p]
                want = a[np.lexsort((a, -lp[a]))][:n]
                assert ids.dtype == np.int64 and logp.dtype == np.float64 and len(ids) == len(logp) == min(n, len(a))
                assert sorted(ids.tolist()) == sorted(want.tolist()), (name, p, n)      # exactly the oracle's best allowed words
                assert np.all(np.diff(logp) <= 0)
                np.testing.assert_allclose(logp, lp[ids], rtol=0, atol=1e-5)
                if n == 6:
                    seqs += [list(prompts[p][1:]) + [int(w)] for w in ids]
                    lps += logp.tolist()
            if n == 6 and seqs:
                sc = model.score(seqs, start)
                np.testing.assert_allclose([-s[-1] for s in sc], lps, rtol=0, atol=1e-5)
    # completion: N = 4, B = 6, the first word within the two-kana set
    N, B = 4, 6
    prefixes = _prefixes(R)[1]
    sets = [index.lookup(x) for x in prefixes]
    order = np.argsort(-np.array([len(p) for p in prompts]), kind="stable")
    live = [i for i in order if len(sets[i])]
    bp_parent, bp_word, bp_nll, score = model._completer().run([np.asarray(prompts[i]) for i in live], N, B, None,
                                                               first_sets=[sets[i] for i in live])
    agree = amb = 0
    for p, i in enumerate(live):
        a, b = _follow(lm, prompts[i], sets[i], bp_parent, bp_word, bp_nll, score, p, N, B)
        agree += a
        amb += b
    assert amb <= max(1, (agree + amb) // 20), (agree, amb)
    res = model.complete_reading(prompts, prefixes, N, beam_width=B)
    seqs, tots = [], []
    for p, hyps in enumerate(res):
        assert len(hyps) == (B if len(sets[p]) else 0)
        assert [h[2] for h in hyps] == sorted(h[2] for h in hyps)
        for ids, nll, tot in hyps:
            assert len(ids) == len(nll) == N and np.isfinite(tot) and int(ids[0]) in set(sets[p].tolist())
            np.testing.assert_allclose(nll.sum(), tot, rtol=0, atol=1e-9)
            seqs.append(list(prompts[p][1:]) + list(ids))
            tots.append(tot)
    for s, tot in zip(model.score(seqs, start), tots):
        assert abs(s[-N:].sum() - tot) <= TOK_ATOL * N, (s[-N:].sum(), tot)
    return model, prompts, index


@pytest.mark.parametrize("name", ["small-vtable", "small-tied-sn", "small-dsoftmax", UNTIED_F32,
                                  # V = 2 003 cut at 501 / 1 203: the last 16-byte chunk of a logit row, and of the bit mask's four
                                  # bits per chunk, is partial
                                  "odd-vtable", "odd-tied", "odd-tied-sn", "odd-dsoftmax", "odd-untied", "oddw-vtable", "odd-untied@f32"])
def test_reading_prediction_matches_oracle(name, fx, monkeypatch):
    _e2e_reading(name, fx, monkeypatch, R=24)


def test_reading_prediction_mid_vtable_against_oracle(fx, monkeypatch):
    _e2e_reading("mid-vtable", fx, monkeypatch, R=3)


def test_small_and_empty_sets(fx):
    f = fx("small-vtable")
    model = load_model(f["root"])
    prompts = ragged_prompts(4, model.dev.V, seed=5)
    index = model.reading_index()
    three = index.lookup(KANA[2])[:3]
    allowed = [three, np.array([], dtype=np.int64), None, three[:1]]
    top = model.predict_top(prompts, n=6, allowed=allowed)
    assert [len(t[0]) for t in top] == [3, 0, 6, 1]
    assert sorted(top[0][0].tolist()) == three.tolist() and top[3][0].tolist() == three[:1].tolist()
    free = model.predict_top(prompts, n=6)
    assert np.array_equal(top[2][0], free[2][0]) and np.array_equal(top[2][1], free[2][1])
    one = model.complete(prompts, 1, beam_width=6, first_allowed=allowed)
    assert [len(r) for r in one] == [3, 0, 6, 1]                              # at most 3 first words, the padding dropped
    assert [h[0][0] for h in one[0]] == top[0][0].tolist()
    res = model.complete(prompts, 4, beam_width=6, first_allowed=allowed)
    assert res[1] == [] and [len(r) for r in res] == [6, 0, 6, 6]             # frame 1: the live hypotheses offer a full beam
    for r, a in ((res[0], three), (res[3], three[:1])):
        assert all(np.isfinite(h[2]) and len(h[0]) == 4 and int(h[0][0]) in a.tolist() for h in r)
    assert len(set(int(h[0][0]) for h in res[0])) <= 3
    with pytest.raises(ValueError):
        model.predict_top(prompts, n=6, allowed=[None, None, None, [model.dev.V]])
    with pytest.raises(ValueError):
        model.predict_reading(prompts, KANA[0])                               # one string per context
    assert model.complete_reading([prompts[0]], [KANA[40]], 3) == [[]]         # a prefix no word has


def test_odd_vocabulary_last_word_and_row_counts(fx):
    """V = 2 003.  A set that holds only word 2 002 -- the one word of the last, partial chunk -- selects exactly that word, with the
    oracle's log p; sets on both sides of every segment cut; calls of 1, 31, 32 and 33 contexts give what the same contexts give inside a
    call of 64"""
    f = fx("odd-vtable")
    model = load_model(f["root"])
    V = model.dev.V
    assert V == 2003
    prompts = ragged_prompts(64, V, seed=23, lo=1, hi=7)
    lm = oracle_lm(f["root"])
    last = np.array([V - 1], dtype=np.int64)
    cuts = np.array([0, 500, 501, 1202, 1203, 2002], dtype=np.int64)
    tail = np.arange(1996, V, dtype=np.int64)                        # the last full chunk and the partial one
    allowed = [(last, cuts, tail, None)[p % 4] for p in range(64)]
    top = model.predict_top(prompts, n=6, allowed=allowed)
    for p in range(64):
        lp = _oracle_logp(lm, prompts[p])[2]
        ids, logp = top[p]
        if allowed[p] is None:
            a = np.arange(V)
        else:
            a = allowed[p]
        want = a[np.lexsort((a, -lp[a]))][:6]
        assert len(ids) == min(6, len(a)), p
        assert sorted(ids.tolist()) == sorted(want.tolist()), (p, ids, want)
        np.testing.assert_allclose(logp, lp[ids], rtol=0, atol=1e-5)
        if p % 4 == 0:
            assert ids.tolist() == [V - 1]
    for n in (1, 31, 32, 33):
        got = model.predict_top(prompts[:n], n=6, allowed=allowed[:n])
        assert len(got) == n
        for p in range(n):
            assert np.array_equal(got[p][0], top[p][0]), (n, p)
            np.testing.assert_allclose(got[p][1], top[p][1], rtol=0, atol=1e-9)
    # the first generated word of a completion inside the one-word set
    res = model.complete(prompts[:8], 3, beam_width=4, first_allowed=[last] * 8)
    for hyps in res:
        assert len(hyps) == 4 and all(int(h[0][0]) == V - 1 and np.isfinite(h[2]) for h in hyps)


@pytest.mark.parametrize("name", ["small-vtable", "small-untied"])
def test_unchanged_paths_cuts_and_neighbours(name, fx):
    f = fx(name)
    model = load_model(f["root"])
    prompts = ragged_prompts(23, model.dev.V, seed=11, lo=1, hi=9)
    n = 12
    top = model.predict_top(prompts, n=n)
    same = model.predict_top(prompts, n=n, allowed=[None] * len(prompts))       # the masked op, every row of set -1
    for a, b in zip(top, same):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    index = model.reading_index()
    has = np.zeros(model.dev.V, dtype=bool)
    has[index.lookup("")] = True
    every = model.predict_reading(prompts, [""] * len(prompts), n=n)
    wide = model.predict_top(prompts, n=n + 2)                                 # at most <unk> and <eos> drop out
    for a, b in zip(every, wide):
        keep = has[b[0]]
        assert np.array_equal(a[0], b[0][keep][:n]) and np.array_equal(a[1], b[1][keep][:n])

    def same_hyps(a, b, exact=False):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            assert np.array_equal(x[0], y[0])
            if exact:
                assert np.array_equal(x[1], y[1]) and x[2] == y[2]
            else:
                np.testing.assert_allclose(x[1], y[1], rtol=0, atol=1e-9)
                assert abs(x[2] - y[2]) <= 1e-9

    B, N = 7, 5
    prefixes = [KANA[p % 12] for p in range(len(prompts))]
    run = lambda ps, rs, **kw: model.complete_reading(ps, rs, N, beam_width=B, n_best=4, **kw)
    res = run(prompts, prefixes)
    assert all(len(r) == 4 for r in res)
    for other, exact in ((run(prompts, prefixes), True), (run(prompts, prefixes, max_rows=3 * B), False), (run(prompts, prefixes, max_rows=1), False)):
        for a, b in zip(res, other):
            same_hyps(a, b, exact)
    for r in (0, 9, 22):                                                       # alone in its call
        same_hyps(res[r], run([prompts[r]], [prefixes[r]])[0])
    tops = model.predict_reading(prompts, prefixes, n=n)
    for r in (0, 9, 22):
        alone = model.predict_reading([prompts[r]], [prefixes[r]], n=n, max_rows=1)[0]
        assert np.array_equal(tops[r][0], alone[0])
        np.testing.assert_allclose(tops[r][1], alone[1], rtol=0, atol=1e-9)


def test_complete_cli_with_reading(fx, capsys):
    from jlm_amd import complete as comp_mod
    f = fx("small-vtable")
    lex = f["lexicon"]
    reading = {w.split("/")[0]: reading_of(w) for w, _c in lex if reading_of(w) is not None}
    prompt = " ".join(w for w, _c in lex[3:5])
    head = " ".join(w.split("/")[0] for w, _c in lex[3:5])
    hira = chr(ord(KANA[4]) - 0x60)                                            # typed in hiragana
    res = comp_mod.main(["--root", f["root"], "-e", "1", "--prompt", prompt, "--top", "5", "--reading", hira])
    out = _lines(capsys)
    assert len(out) == 5 and len(res) == 1
    for line, lp in zip(out, res[0][1]):
        text, nl = line.split("\t")
        assert text.startswith(head + " ") and reading[text[len(head) + 1:]].startswith(KANA[4])
        assert abs(float(nl) + lp) < 1e-3
    res = comp_mod.main(["--root", f["root"], "-e", "1", "--prompt", prompt, "--top", "64", "--reading", KANA[4], "--exact"])
    out = _lines(capsys)
    assert 4 <= len(out) == len(res[0][0]) <= 15                               # every word read exactly so
    assert all(reading[line.split("\t")[0][len(head) + 1:]] == KANA[4] for line in out)
    res = comp_mod.main(["--root", f["root"], "-e", "1", "--prompt", prompt, "--words", "3", "-b", "6", "--n-best", "3", "--reading", KANA[4]])
    out = _lines(capsys)
    assert len(out) == 3 and len(res) == 1
    for line, h in zip(out, res[0]):
        text, tot = line.split("\t")
        words = text[len(head) + 1:].split(" ")
        assert len(words) == 3 and reading[words[0]].startswith(KANA[4])
        assert abs(float(tot) - h[2]) < 1e-3
