"""GPU: next-word prediction and beam-search completion (LSTM_Model.predict_top / complete, python -m jlm_amd.complete; csrc
jlm_complete_frames + topk_rows_kernel + beam_merge_kernel).

Kernel level: torch.ops.jlm.topk_rows over logits the test writes gives exactly the ids of a numpy stable ranking of the same f32 rows
(complete.topk_reference), nll within 1e-6 of the f64 lse - y (-y exactly on self-normalised rows), top-1 = sample_rows' greedy
draw; torch.ops.jlm.beam_merge fed the kernel's own lists equals complete.merge_reference bit for bit.

End to end, against the oracle's OracleLM (oracle/jlm_oracle.py, float64) teacher-forced on the device's beams: at every frame the
kept set is the oracle's top-B from the device's parents, except where the oracle's gap at the cut is under TOL_E2E (counted, asserted
rare); totals within TOK_ATOL per word of the oracle and of score()."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
from jlm_amd import _lib, complete as C, ops as _ops                                      # noqa: E402
from tests.gpu_rows import UNTIED_F32, fixture_model, load_model, lse, oracle_lm, ragged_prompts     # noqa: E402

pytestmark = pytest.mark.gpu

TOK_ATOL = 1e-5
TOL_E2E = 1e-4          # the device's logits differ from float64 ones by ~1e-6: a cut this close is ambiguous


def _dev():
    return _lib.require_gpu()


def _topk(y, k, self_norm=False):
    """one jlm_topk_rows launch over y [R, n_cols] (f32 numpy) -> (ids [R, k], nll [R, k], flags)"""
    dev = _dev()
    R, n = y.shape
    ld = (n + 3) // 4 * 4
    yp = np.full((R, ld), np.nan, dtype=np.float32)        # the padding is never read as a word
    yp[:, :n] = y
    yt = torch.from_numpy(yp).to(dev)
    ids = torch.full((R, k), -7, device=dev, dtype=torch.int32)
    nll = torch.zeros((R, k), device=dev, dtype=torch.float64)
    flags = torch.zeros(1, device=dev, dtype=torch.int32)
    _ops.backend().topk_rows(yt, ld, n, R, k, bool(self_norm), ids, nll, k, flags)
    torch.cuda.synchronize()
    return ids.cpu().numpy(), nll.cpu().numpy(), int(flags.cpu()[0])


def _greedy(y, self_norm=False):
    dev = _dev()
    R, n = y.shape
    ld = (n + 3) // 4 * 4
    yp = np.zeros((R, ld), dtype=np.float32)
    yp[:, :n] = y
    word = torch.zeros(R, device=dev, dtype=torch.int32)
    ids = torch.zeros(R, device=dev, dtype=torch.int32)
    nll = torch.zeros(R, device=dev, dtype=torch.float64)
    _ops.backend().sample_rows(torch.from_numpy(yp).to(dev), ld, n, R, None, 0.0, 0, 0, None, None, None, -1, bool(self_norm), word,
                               ids, nll, None)
    torch.cuda.synchronize()
    return ids.cpu().numpy()


def _check_rows(y, k, self_norm=False):
    ids, nll, fl = _topk(y, k, self_norm)
    assert fl == 0
    for r in range(y.shape[0]):
        want_ids, want_nll = C.topk_reference(y[r], k, self_norm)
        assert ids[r].tolist() == want_ids.tolist(), (r, ids[r][:8], want_ids[:8])
        if self_norm:
            assert np.array_equal(nll[r], -y[r, want_ids].astype(np.float64))
        else:
            np.testing.assert_allclose(nll[r], want_nll, rtol=0, atol=1e-6)
    assert np.array_equal(ids[:, 0], _greedy(y, self_norm))
    return ids, nll


@pytest.mark.parametrize("n_cols", [1, 2, 63, 64, 65, 1000, 50000, 100003])
@pytest.mark.parametrize("k", [1, 2, 10, 33, 64])
def test_topk_rows_random_logits(n_cols, k):
    if k > n_cols:
        with pytest.raises(RuntimeError):                                   # k > n_cols is refused
            _topk(np.zeros((2, n_cols), dtype=np.float32), k)
        return
    rng = np.random.RandomState(n_cols * 100 + k)
    R = 24 if n_cols <= 1000 else 6
    y = (rng.standard_normal((R, n_cols)) * 3).astype(np.float32)
    _check_rows(y, k)
    _check_rows(y, k, self_norm=True)


@pytest.mark.parametrize("k", [1, 10, 64])
def test_topk_rows_special_rows(k):
    rng = np.random.RandomState(k)
    n = 5003
    rows = [np.full(n, 1.25, dtype=np.float32),                              # all equal: ids 0 .. k-1
            np.arange(n, dtype=np.float32) * 1e-3,                           # ascending: every word beats the list so far
            -np.arange(n, dtype=np.float32) * 1e-3,                          # descending
            rng.randint(-2, 3, size=n).astype(np.float32)]                   # five values: ties everywhere
    straddle = rng.standard_normal(n).astype(np.float32)
    top = np.sort(rng.choice(n, size=k + 5, replace=False))
    straddle[top[:k - 1]] = 8.0
    straddle[top[k - 1:]] = 7.0                                              # six equal logits at the k-th place
    rows.append(straddle)
    dom = rng.standard_normal(n).astype(np.float32)
    dom[rng.randint(0, n)] = 60.0                                            # one dominant word
    rows.append(dom)
    y = np.stack(rows)
    ids, _nll = _check_rows(y, k)
    assert ids[0].tolist() == list(range(k))
    _check_rows(y, k, self_norm=True)


def test_topk_rows_non_finite_sets_flag():
    y = np.random.RandomState(2).standard_normal((4, 2000)).astype(np.float32)
    y[2, 777] = np.nan
    ids, nll, fl = _topk(y, 10)
    assert fl & 1
    assert np.all(ids[2] == -1) and np.all(np.isnan(nll[2]))
    ok = [0, 1, 3]
    for r in ok:
        assert ids[r].tolist() == C.topk_reference(y[r], 10)[0].tolist()
    y[2, 777] = np.inf
    assert _topk(y, 10)[2] & 1
    assert _topk(y, 10, self_norm=True)[2] & 1
    y[2, 777] = -np.inf                                                      # a -inf logit is a word of probability 0
    assert _topk(y, 10)[2] == 0


def _merge(ci, cn, score, finished, B, NP, first, stop_id):
    dev = _dev()
    R = NP * B
    i32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
    f64 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    word, prev = i32(np.zeros(R)), i32(np.zeros(R))
    sc, fin = f64(score), i32(finished)
    bpp, bpw, bpn = i32(np.zeros(R)), i32(np.zeros(R)), f64(np.zeros(R))
    _ops.backend().beam_merge(i32(ci), f64(cn), B, NP, bool(first), int(stop_id), word, prev, sc, fin, bpp, bpw, bpn)
    torch.cuda.synchronize()
    return dict(word=word.cpu().numpy(), prev=prev.cpu().numpy(), score=sc.cpu().numpy(), finished=fin.cpu().numpy(),
                bp_parent=bpp.cpu().numpy(), bp_word=bpw.cpu().numpy(), bp_nll=bpn.cpu().numpy())


@pytest.mark.parametrize("B", [1, 2, 5, 17, 64])
def test_beam_merge_matches_restatement(B):
    rng = np.random.RandomState(B)
    NP, V = 7, 300
    R = NP * B
    # logits on a coarse grid: equal nll within a row, and equal scores across rows
    y = (rng.randint(-6, 7, size=(R, V)) * 0.5).astype(np.float32)
    y[1::2] = y[0:R - 1:2]                 # neighbouring rows alike: equal scores across parents too
    ci, cn, fl = _topk(y, B)
    assert fl == 0
    for first in (True, False):
        for stop_id in (-1, int(ci[0, 0])):
            score = (rng.randint(0, 4, size=R) * 0.25).astype(np.float64)
            finished = (rng.rand(R) < 0.25).astype(np.int32)
            got = _merge(ci, cn, score, finished, B, NP, first, stop_id)
            want = C.merge_reference(ci, cn, score, finished, B, NP, first, stop_id)
            for key in ("bp_parent", "bp_word", "score", "finished", "prev", "word", "bp_nll"):
                assert np.array_equal(got[key], want[key]), (key, first, stop_id)


# ------------------------------------------------------------------------------------------------------------- end to end
SMALL = ["small-tied", "small-untied", "small-dsoftmax", "small-vtable", "small-tied-sn", "small-untied-sn", "small-dsoftmax-sn",
         "small-vtable-sn", "small-char", "peaked20-vtable"]


def _device_beams(model, prompts, N, B, stop_id=None):
    """one device call over the prompts (sorted longest first here) -> (order, bp_parent, bp_word, bp_nll, score)"""
    order = np.argsort(-np.array([len(p) for p in prompts]), kind="stable")
    comp = model._completer()
    bp_parent, bp_word, bp_nll, score = comp.run([np.asarray(prompts[i]) for i in order], N, B, stop_id)
    return order, bp_parent, bp_word, bp_nll, score


def oracle_follow(lm, prompt, bp_parent, bp_word, bp_nll, score, p, N, B, stop_id=None):
    """the oracle teacher-forced on prompt p's device beams: per frame the oracle's top-B from the device's parents must be the device's
    kept set unless the oracle's gap at the cut is under TOL_E2E.  -> (agreeing frames, ambiguous frames)"""
    sn = lm.config["self_norm"]
    h, c = lm.zero_state(1)
    for w in prompt:
        h, c = lm.lstm_cell(np.array([w]), h, c)
    beam = [dict(h=h[0], c=c[0], s=0.0, fin=False, n=0)]
    agree = amb = 0
    for k in range(N):
        H = np.stack([b["h"] for b in beam])
        Y = lm.project(H)
        cands = []
        for j, b in enumerate(beam):
            if b["fin"]:
                cands.append((b["s"], j, -1))
                continue
            y = Y[j]
            nll = -y if sn else lse(y) - y
            tot = b["s"] + nll
            top = np.argsort(tot, kind="stable")[:B + 1]
            cands.extend((float(tot[w]), j, int(w)) for w in top)
        cands.sort()
        q = p * B + np.arange(B)
        dev_set = set(zip(bp_parent[k, q].tolist(), bp_word[k, q].tolist()))
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
            par = beam[j]
            if w < 0:
                assert par["fin"] and n == 0.0
                nb.append(dict(par))
                continue
            y = Y[j]
            on = -y[w] if sn else lse(y) - y[w]
            assert abs(n - on) <= TOK_ATOL, (k, i, n, on)
            h2, c2 = lm.lstm_cell(np.array([w]), par["h"][None], par["c"][None])
            nb.append(dict(h=h2[0], c=c2[0], s=par["s"] + on, fin=stop_id is not None and w == stop_id, n=par["n"] + 1))
        beam = nb
    for i in range(B):
        assert abs(score[p * B + i] - beam[i]["s"]) <= TOK_ATOL * max(1, beam[i]["n"]), (p, i, score[p * B + i], beam[i]["s"])
    return agree, amb


def _e2e(name, fx, monkeypatch, R, N, B, stop_id=None, seed=0):
    f, model = fixture_model(fx, name, monkeypatch)
    V = model.dev.V
    prompts = ragged_prompts(R, V, seed=len(name) + seed)
    order, bp_parent, bp_word, bp_nll, score = _device_beams(model, prompts, N, B, stop_id)
    lm = oracle_lm(f["root"])
    agree = amb = 0
    for p, i in enumerate(order):
        a, b = oracle_follow(lm, prompts[i], bp_parent, bp_word, bp_nll, score, p, N, B, stop_id)
        agree += a
        amb += b
    assert amb <= max(1, (agree + amb) // 20), (agree, amb)
    # the public form: totals = score() of the output sequences
    res = model.complete(prompts, N, beam_width=B, stop_id=stop_id)
    seqs, tots = [], []
    for p, hyps in zip(prompts, res):
        assert len(hyps) == B
        assert [h[2] for h in hyps] == sorted(h[2] for h in hyps)
        for ids, nll, tot in hyps:
            assert ids.dtype == np.int64 and nll.dtype == np.float64 and len(ids) == len(nll) >= 1
            assert stop_id is not None or len(ids) == N
            if stop_id is not None and len(ids) < N:
                assert ids[-1] == stop_id
            np.testing.assert_allclose(nll.sum(), tot, rtol=0, atol=1e-9)
            seqs.append(list(p[1:]) + list(ids))
            tots.append((tot, len(ids)))
    sc = model.score(seqs, prompts[0][0])
    for s, (tot, n) in zip(sc, tots):
        assert abs(s[-n:].sum() - tot) <= TOK_ATOL * n, (s[-n:].sum(), tot)
    return model, prompts, res


# V = 2 003 cut at 501 / 1 203 (jlm_amd/synth.py): ld_logits > V, every segment's logits start at an unaligned column
ODD = ["odd-tied", "odd-untied", "odd-dsoftmax", "odd-vtable", "odd-tied-sn", "odd-untied-sn", "odd-dsoftmax-sn", "odd-vtable-sn",
       "oddw-vtable", "odd-untied@f32"]


@pytest.mark.parametrize("name", SMALL + [UNTIED_F32] + ODD)
def test_complete_matches_oracle(name, fx, monkeypatch):
    _e2e(name, fx, monkeypatch, R=6, N=5, B=6)


def test_complete_mid_vtable_against_oracle(fx, monkeypatch):
    _e2e("mid-vtable", fx, monkeypatch, R=3, N=3, B=4)


def test_complete_stop_id_against_oracle(fx, monkeypatch):
    f = fx("small-vtable")
    model = load_model(f["root"])
    prompts = ragged_prompts(8, model.dev.V, seed=len("small-vtable") + 4)          # _e2e's prompts for seed 4
    res = model.complete(prompts, 6, beam_width=5)
    stop = int(np.bincount(np.concatenate([h[0][:3] for r in res for h in r])).argmax())    # a word the beams reach early
    _m, _p, res2 = _e2e("small-vtable", fx, monkeypatch, R=8, N=6, B=5, stop_id=stop, seed=4)
    assert any(len(h[0]) < 6 for r in res2 for h in r)                 # some hypothesis finished and was carried


@pytest.mark.parametrize("name", ["small-vtable", "small-tied-sn", "small-char", "peaked20-vtable"])
def test_beam1_is_greedy_and_predict_top(name, fx):
    f = fx(name)
    model = load_model(f["root"])
    prompts = ragged_prompts(20, model.dev.V, seed=7, hi=8)
    greedy, gnll = model.generate(prompts, 7, temperature=0.0)
    res = model.complete(prompts, 7, beam_width=1)
    top = model.predict_top(prompts, n=1)
    for r in range(20):
        ids, nll, tot = res[r][0]
        assert np.array_equal(ids, greedy[r]), r
        np.testing.assert_allclose(nll, gnll[r], rtol=0, atol=1e-6)
        assert top[r][0].tolist() == [greedy[r][0]]
        np.testing.assert_allclose(-top[r][1][0], gnll[r][0], rtol=0, atol=1e-6)
    # predict_top(c, n) is frame 0 of complete(c, 1, beam_width=n)
    n = 12
    top = model.predict_top(prompts, n=n)
    one = model.complete(prompts, 1, beam_width=n)
    for r in range(20):
        assert top[r][0].dtype == np.int64 and top[r][1].dtype == np.float64 and len(top[r][0]) == n
        assert top[r][0].tolist() == [h[0][0] for h in one[r]]
        assert np.array_equal(top[r][1], -np.array([h[1][0] for h in one[r]]))
        assert np.all(np.diff(top[r][1]) <= 0)


@pytest.mark.parametrize("name", ["small-vtable", "small-untied", "small-char"])
def test_complete_repeat_cuts_and_neighbours(name, fx):
    f = fx(name)
    model = load_model(f["root"])
    prompts = ragged_prompts(23, model.dev.V, seed=11, lo=1, hi=9)
    B, N = 7, 5

    def same(a, b, exact=False):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            assert np.array_equal(x[0], y[0])
            if exact:
                assert np.array_equal(x[1], y[1]) and x[2] == y[2]
            else:
                np.testing.assert_allclose(x[1], y[1], rtol=0, atol=1e-9)
                assert abs(x[2] - y[2]) <= 1e-9

    res = model.complete(prompts, N, beam_width=B, n_best=4)
    assert all(len(r) == 4 for r in res)
    same_all = lambda r1, r2, exact=False: [same(a, b, exact) for a, b in zip(r1, r2)]
    same_all(res, model.complete(prompts, N, beam_width=B, n_best=4), exact=True)        # bit-identical run to run
    same_all(res, model.complete(prompts, N, beam_width=B, n_best=4, max_rows=3 * B))    # cut into calls of 3 prompts
    same_all(res, model.complete(prompts, N, beam_width=B, n_best=4, max_rows=1))        # one prompt per call
    for r in (0, 9, 22):                                                                 # alone in its call
        same(res[r], model.complete([prompts[r]], N, beam_width=B, n_best=4)[0])


@pytest.mark.parametrize("n_prompts,B", [(1, 1), (1, 64), (33, 3)])
def test_complete_odd_vocabulary_row_counts(n_prompts, B, fx):
    """V = 2 003: a call of n_prompts x beam rows gives what the same prompts give inside a call of 40 prompts"""
    f = fx("odd-vtable")
    model = load_model(f["root"])
    assert model.dev.V == 2003
    prompts = ragged_prompts(40, 2003, seed=17, lo=1, hi=7)
    N = 4
    big = model.complete(prompts, N, beam_width=B)
    got = model.complete(prompts[:n_prompts], N, beam_width=B)
    assert len(got) == n_prompts
    for a, b in zip(got, big):
        assert len(a) == len(b) == B
        for x, y in zip(a, b):
            assert np.array_equal(x[0], y[0])
            np.testing.assert_allclose(x[1], y[1], rtol=0, atol=1e-9)
            assert abs(x[2] - y[2]) <= 1e-9


def test_complete_errors(fx):
    f = fx("small-tied")
    model = load_model(f["root"])
    V = model.dev.V
    for kw in (dict(prompts=[[V]]), dict(prompts=[[]]), dict(n_words=0), dict(beam_width=65), dict(beam_width=0),
               dict(n_best=11), dict(stop_id=V)):
        args = dict(prompts=[[1]], n_words=3, beam_width=10)
        args.update(kw)
        with pytest.raises(ValueError):
            model.complete(**args)
    with pytest.raises(ValueError):
        model.predict_top([[1]], n=65)
    assert model.complete([], 3) == []


def _lines(capsys):
    """the CLI's result lines (the model loader announces itself on stdout first)"""
    return [l for l in capsys.readouterr().out.split("\n") if l and not l.startswith("LSTM model:")]


@pytest.mark.parametrize("name", ["small-vtable", "small-char"])
def test_complete_cli(name, fx, capsys, tmp_path):
    from jlm_amd import complete as comp_mod
    f = fx(name)
    lex = f["lexicon"]
    prompt = " ".join(w for w, _c in lex[3:5])
    head = "".join(w.split("/")[0] for w, _c in lex[3:5]) if name == "small-char" else " ".join(w.split("/")[0] for w, _c in lex[3:5])
    # next-word mode
    res = comp_mod.main(["--root", f["root"], "-e", "1", "--prompt", prompt, "--top", "5"])
    out = _lines(capsys)
    assert len(out) == 5 and len(res) == 1
    for line, lp in zip(out, res[0][1]):
        text, nl = line.split("\t")
        assert text.startswith(head)
        assert abs(float(nl) + lp) < 1e-3
    # completion mode, two prompts from a file, stopping at <eos>
    p = tmp_path / "prompts.txt"
    p.write_text(prompt + "\n" + " ".join(w for w, _c in lex[6:7]) + "\n", encoding="utf-8")
    res = comp_mod.main(["--root", f["root"], "-e", "1", "--file", str(p), "--words", "4", "-b", "6", "--n-best", "3",
                         "--stop-at-eos"])
    out = _lines(capsys)
    assert len(res) == 2 and len(out) == 6
    assert all(line.startswith(head) for line in out[:3])
    for line, h in zip(out, [h for r in res for h in r]):
        assert abs(float(line.split("\t")[1]) - h[2]) < 1e-3
