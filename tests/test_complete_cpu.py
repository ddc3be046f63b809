"""CPU-only: the host side of next-word prediction and beam-search completion (jlm_amd/complete.py) -- argument checks, the row plan,
the numpy restatements of the row selection and the merge key the kernels implement, the backtrace and stop truncation, and the new
C entry points in the ctypes table."""
import numpy as np
import pytest

from jlm_amd import _lib, complete as C


def test_check_args():
    V = 100
    prompts, n_best = C.check_args([[1, 2], [3]], 4, 10, None, None, V)
    assert n_best == 10 and [p.tolist() for p in prompts] == [[1, 2], [3]]
    assert C.check_args([[1]], 1, 64, 64, 5, V)[1] == 64
    bad = [dict(n_words=0), dict(n_words=1.5), dict(n_words=True), dict(beam_width=0), dict(beam_width=65), dict(beam_width=2.0),
           dict(n_best=0), dict(n_best=11), dict(prompts=[[]]), dict(prompts=[[V]]), dict(prompts=[[-1]]), dict(stop_id=V),
           dict(stop_id=-1)]
    for kw in bad:
        args = dict(prompts=[[1]], n_words=3, beam_width=10, n_best=None, stop_id=None, V=V)
        args.update(kw)
        with pytest.raises(ValueError):
            C.check_args(**args)
    with pytest.raises(ValueError):                      # the beam is bounded by the vocabulary too
        C.check_args([[1]], 1, 9, None, None, 8)


def test_plan_prompts_never_splits_a_beam():
    lens = [2, 5, 1, 5, 3, 1, 4]
    for B, max_rows in ((10, 30), (10, 25), (10, 9), (1, 3), (64, 2560)):
        chunks = C.plan_prompts(lens, B, max_rows)
        per = max(1, max_rows // B)
        got = np.concatenate([c["idx"] for c in chunks])
        assert sorted(got.tolist()) == list(range(len(lens)))          # every prompt once
        assert all(len(c["idx"]) <= per for c in chunks)               # a chunk's rows: whole beams, within the budget (or one prompt)
        assert [lens[i] for i in got] == sorted(lens, reverse=True)    # longest first, across the cut
        for c in chunks:
            assert c["n_live"][-1] == len(c["idx"])
    # cut invariance of the order: the chunks of a smaller budget are a refinement of the one-call order
    one = C.plan_prompts(lens, 4, 10 ** 6)[0]["idx"].tolist()
    cut = np.concatenate([c["idx"] for c in C.plan_prompts(lens, 4, 8)]).tolist()
    assert one == cut
    with pytest.raises(ValueError):
        C.plan_prompts(lens, 4, 0)


def test_topk_reference_ties_and_full_row():
    y = np.array([0.5, 3.0, -1.0, 3.0, 3.0, 2.0], dtype=np.float32)
    ids, nll = C.topk_reference(y, 4)
    assert ids.tolist() == [1, 3, 4, 5]                 # equal logits: lower id first
    yd = y.astype(np.float64)
    lse = np.log(np.exp(yd).sum())
    np.testing.assert_allclose(nll, lse - yd[[1, 3, 4, 5]], rtol=0, atol=1e-12)
    ids, nll = C.topk_reference(y, 6)                   # k = n_cols: the whole row ranked
    assert ids.tolist() == [1, 3, 4, 5, 0, 2]
    assert np.all(np.diff(nll) >= 0)
    ids, nll = C.topk_reference(y, 2, self_norm=True)
    assert ids.tolist() == [1, 3] and nll.tolist() == [-3.0, -3.0]
    assert C.topk_reference(np.array([7.0], dtype=np.float32), 1)[0].tolist() == [0]
    # top-1 is the greedy draw's argmax (lowest id on a tie)
    rng = np.random.RandomState(0)
    for _ in range(20):
        z = rng.randint(0, 4, size=50).astype(np.float32)
        assert C.topk_reference(z, 1)[0][0] == int(np.argmax(z))


def _brute(ys, score, finished, B, first, stop_id=-1):
    """the merge over EVERY word of every parent row (not just the per-row lists): the key the lists must reproduce"""
    cands = []
    for j in range(1 if first else B):
        ps = 0.0 if first else score[j]
        if not first and finished[j]:
            cands.append((ps, j, -1))
            continue
        _ids, nll = C.topk_reference(ys[j], len(ys[j]))
        for w, n in zip(_ids, nll):
            cands.append((ps + n, j, int(w)))
    cands.sort()
    return cands[:B]


def test_merge_reference_key_carries_and_first_frame():
    B = 3
    # two prompts; rows' lists [rows, B]
    ci = np.array([[5, 2, 7], [1, 0, 9], [4, 6, 3], [8, 3, 2], [2, 5, 1], [7, 0, 4]], dtype=np.int32)
    cn = np.array([[0.5, 1.0, 1.0], [0.25, 0.75, 2.0], [0.1, 0.2, 0.3], [1.0, 1.0, 1.0], [0.5, 0.5, 3.0], [0.0, 2.0, 2.0]])
    score = np.array([1.0, 1.25, 5.0, 0.0, 0.0, 0.5])
    finished = np.array([0, 0, 1, 0, 0, 0], dtype=np.int32)
    out = C.merge_reference(ci, cn, score, finished, B, 2, first=False, stop_id=4)
    # prompt 0: candidates 1.5 (0,5) 2.0 (0,2) 2.0 (0,7) 1.5 (1,1) 2.0 (1,0) 3.25 (1,9) carry 5.0 (2) -> (0,5) (1,1) (0,2)
    assert out["bp_parent"][:3].tolist() == [0, 1, 0]
    assert out["bp_word"][:3].tolist() == [5, 1, 2]
    assert out["score"][:3].tolist() == [1.5, 1.5, 2.0]
    assert out["prev"][:3].tolist() == [0, 1, 0]
    # prompt 1: 1.0 (0,8) (0,3) (0,2); 0.5 (1,2) (1,5); 3.5; 0.5 (2,7); 2.5 (2,0) (2,4) -> (1,2) (1,5) (2,7)
    assert out["bp_parent"][3:].tolist() == [1, 1, 2]
    assert out["bp_word"][3:].tolist() == [2, 5, 7]
    assert out["prev"][3:].tolist() == [4, 4, 5]
    # a carry ranks by the same key, word -1, nll 0; stop_id marks a new hypothesis finished
    score2 = np.array([0.1, 9.0, 9.0, 0.0, 0.0, 0.0])
    fin2 = np.array([1, 0, 0, 0, 0, 0], dtype=np.int32)
    out = C.merge_reference(ci, cn, score2, fin2, B, 2, first=False, stop_id=4)
    assert out["bp_word"][0] == -1 and out["bp_parent"][0] == 0 and out["score"][0] == 0.1 and out["finished"][0] == 1
    assert out["bp_nll"][0] == 0.0 and out["word"][0] == 4
    assert out["bp_word"][:3].tolist() == [-1, 4, 6] and out["bp_parent"][:3].tolist() == [0, 2, 2]
    assert out["finished"][:3].tolist() == [1, 1, 0]
    # frame 0: one candidate row per prompt (row p), parent score 0
    out = C.merge_reference(ci, cn, None, None, B, 2, first=True)
    assert out["bp_word"].tolist() == [5, 2, 7, 1, 0, 9]
    assert out["bp_parent"].tolist() == [0] * 6 and out["prev"].tolist() == [0, 0, 0, 1, 1, 1]
    assert out["score"].tolist() == [0.5, 1.0, 1.0, 0.25, 0.75, 2.0]


def test_per_row_lists_are_enough():
    """the merge over per-row top-B lists equals the merge over every word of every row (random rows with many ties)"""
    rng = np.random.RandomState(3)
    for trial in range(30):
        B, V = rng.randint(1, 7), rng.randint(7, 40)
        ys = [rng.randint(-3, 3, size=V).astype(np.float32) * 0.5 for _ in range(B)]
        lists = [C.topk_reference(y, B) for y in ys]
        ci = np.array([l[0] for l in lists], dtype=np.int32)
        cn = np.array([l[1] for l in lists])
        score = rng.randint(0, 3, size=B).astype(np.float64) * 0.25
        finished = (rng.rand(B) < 0.3).astype(np.int32)
        for first in (False, True):
            out = C.merge_reference(ci, cn, score, finished, B, 1, first=first)
            want = _brute(ys, score, finished, B, first)
            got = [(out["score"][i], int(out["bp_parent"][i]), int(out["bp_word"][i])) for i in range(B)]
            assert got == want, (trial, first)


def test_backtrace_and_truncation():
    # one prompt, beam 2, three frames; rank i of frame k at column i
    bp_parent = np.array([[0, 0], [1, 0], [0, 0]], dtype=np.int32)
    bp_word = np.array([[10, 11], [12, 13], [-1, 14]], dtype=np.int32)
    bp_nll = np.array([[0.5, 0.7], [0.1, 0.2], [0.0, 0.4]])
    score = np.array([0.8, 1.1])
    hyps = C.backtrace(bp_parent, bp_word, bp_nll, score, 0, 2, 2, stop_id=12)
    # rank 0: frame 2 carry of frame-1 rank 0 (word 12 from parent 1 = word 11): [11, 12], stopped
    assert hyps[0][0].tolist() == [11, 12] and hyps[0][1].tolist() == [0.7, 0.1] and hyps[0][2] == 0.8
    # rank 1: 14 from frame-1 rank 0 (12 from 11): cut after the stop word
    assert hyps[1][0].tolist() == [11, 12] and hyps[1][2] == 1.1
    hyps = C.backtrace(bp_parent, bp_word, bp_nll, score, 0, 2, 1, stop_id=None)
    assert len(hyps) == 1 and hyps[0][0].tolist() == [11, 12]
    # a second prompt's rows sit behind the first's
    two_p = np.concatenate([bp_parent, bp_parent], axis=1)
    two_w = np.concatenate([bp_word, np.where(bp_word >= 0, bp_word + 100, -1)], axis=1)
    two_n = np.concatenate([bp_nll, bp_nll], axis=1)
    hyps = C.backtrace(two_p, two_w, two_n, np.concatenate([score, score + 1]), 1, 2, 2)
    assert hyps[0][0].tolist() == [111, 112] and hyps[0][1].tolist() == [0.7, 0.1] and hyps[0][2] == 1.8
    assert hyps[1][0].tolist() == [111, 112, 114] and hyps[1][1].tolist() == [0.7, 0.1, 0.4] and hyps[1][2] == 2.1


def test_new_entry_points_in_ctypes_table():
    for n in ("jlm_topk_rows", "jlm_beam_merge", "jlm_complete_frames"):
        assert n in _lib.EXPORTS
    names = [f[0] for f in _lib.CompletePlan._fields_]
    assert names[:4] == ["n_prompts", "beam", "n_prompt", "n_words"] and names[-1] == "flags"
