"""CPU: conversion under a memory -- the yardstick checks itself (tests/decode_memory_cases.py), the doubles of
the two launchers and of the plan field against the float64 definition (tests/fake_memory_edge.py), the host-side search and the
device path over the doubles against the proxy, the launch lists with and without a memory, every refusal, and the command-line
flags."""
import types

import numpy as np
import pytest

from jlm_amd import memory as M
from tests import context_cases as cc
from tests import decode_memory_cases as mc
from tests import fake_memory_edge
from tests.decode_memory_budget import path_atol, score_bars, RTOL

SENTS = mc.sentences()


# ---------------------------------------------------------------------------------------------- the yardstick checks itself
@pytest.mark.parametrize("name", list(cc.MODELS))
def test_memory_oracle_moves_the_result_and_k16_is_separable_often_enough(name):
    """theta = 0.6, lam = 0.5, beam 5: with the whole memory voting (K = 1 024 >= N) the oracle's 1-best differs from the plain oracle's
    on at least 4 of the 12 inputs, and its score is the chain rule's; at K = 16 at least 3 inputs are separable -- every query row's
    16th and 17th float64 scores further apart than twice the end-to-end score bar -- so the fixtures cannot degenerate silently"""
    o = cc.oracle(name)
    ids, keys, words = mc.store(name)
    assert 700 <= len(ids) <= 850 and keys.shape == (len(ids), cc.MODELS[name][1])
    moved = separable = 0
    for text in SENTS:
        plain = o.decode(text, beam_width=5)
        got, sep = mc.memory_decode(o, text, None, name, mc.K_ALL, beam_width=5)
        assert sep                                                         # (K >= N: no boundary, nothing to separate)
        lo, mid, hi = mc.chain_interval(o.model, [cc.EOS], cc.path_ids(o, got[0][1]), keys, words, mc.K_ALL)
        assert lo == mid == hi and abs(got[0][0] - mid) <= 1e-9, (name, text, got[0][0], mid)
        moved += got[0][1] != plain[0][1]
        small, sep = mc.memory_decode(o, text, None, name, mc.K_SMALL, beam_width=5)
        lo, mid, hi = mc.chain_interval(o.model, [cc.EOS], cc.path_ids(o, small[0][1]), keys, words, mc.K_SMALL)
        assert lo <= mid <= hi and abs(small[0][0] - mid) <= 1e-9
        separable += sep
    assert moved >= 4 and separable >= 3, (name, moved, separable)


def test_memory_lm_is_the_definition():
    name = "tied"
    o = cc.oracle(name)
    _ids, keys, words = mc.store(name)
    V = cc.MODELS[name][0]
    for K in (mc.K_SMALL, mc.K_ALL):
        p = mc.MemoryLM(o.model, [cc.EOS, 7, 9], keys, words, K)
        h, c = p.zero_state(1)
        pred, _y, h2, _c2, _a, _b = p.predict([cc.EOS], h, c)
        plain = o.model.predict([9], h, c)[0]
        want = (1 - mc.LAM) * plain[0] + mc.LAM * M.memory_distribution(h2[0], keys, words, mc.THETA, K, V)
        np.testing.assert_allclose(pred[0], want, rtol=1e-12, atol=0)
        assert abs(pred.sum() - 1.0) < 1e-9
        assert len(p.margins) == (1 if K < len(words) else 0)
    bars = score_bars(h2[0], keys, mc.THETA)
    assert bars.shape == (len(words),) and 0 < bars.max() < 2e-4           # (the bar the separable fixture stands on: far below a score)


# ---------------------------------------------------------------------------------------------- the launchers' doubles
def _i32(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32))


def test_patch_double_is_the_definition_and_gather_copies_live_rows():
    import torch
    lib = fake_memory_edge.EdgeLib()
    rng = np.random.RandomState(3)
    B, beam, K, N, J = 2, 3, 8, 5, 4                                        # n_q = 5 < K: entries 5 .. 7 are never read
    n_rows = B * beam
    s = torch.from_numpy(rng.randn(n_rows, K).astype(np.float32))
    s[:, N:] = float("nan")
    words = rng.randint(2, 6, size=(K, n_rows)).astype(np.int32)
    ret = _i32(words)
    cnt, slen, base = _i32([3, 2]), _i32([4, 4]), _i32([0, 3])
    wl, wl_off, wl_idx, wl_out = _i32([2, 3, 4, 9, 5, 2, 3, 9]), _i32([0, 4, 8]), _i32([0, 1]), _i32(np.arange(8))
    y = rng.randn(8, beam).astype(np.float32)
    edge = torch.from_numpy(y.copy())
    part = torch.from_numpy(np.stack([rng.randn(2, n_rows), rng.rand(2, n_rows) + 0.5], axis=2).astype(np.float32))
    lse = torch.full((n_rows,), -7.0, dtype=torch.float64)
    flags = torch.zeros(1, dtype=torch.int32)
    o = lambda t: t.data_ptr()
    lam = 0.25
    args = lambda **kw: list(dict(dict(s=o(s), ld_s=K, ret=o(ret), n_rows=n_rows, N=N, K=K, lam=lam, cnt=o(cnt), slen=o(slen), frame=1, n_sent=B,
                                       beam=beam, wl=o(wl), wl_off=o(wl_off), wl_idx=o(wl_idx), wl_base=0, wl_out=o(wl_out), edge=o(edge),
                                       part=o(part), ld_part=n_rows, n_parts=2, base=o(base), lse=o(lse), flags=o(flags), stream=0), **kw).values())
    for bad in (dict(lam=0.0), dict(lam=1.0), dict(K=0), dict(K=1025), dict(ld_s=K - 1), dict(n_rows=0), dict(n_rows=65536), dict(N=0),
                dict(beam=0), dict(beam=1025), dict(n_sent=65536), dict(s=0), dict(ret=0), dict(base=0), dict(edge=0), dict(n_parts=0),
                dict(lse=0), dict(wl_base=-1), dict(frame=-1)):
        assert lib.jlm_memory_cell_patch(*args(**bad)) == -1 and lib.launches == [], bad
    assert lib.jlm_memory_cell_patch(*args(n_sent=0)) == 0 and lib.launches == []
    assert lib.jlm_memory_cell_patch(*args()) == 0 and lib.launches == ["memory_cell_patch"] and int(flags[0]) == 0
    pv = part.numpy().astype(np.float64)
    got = edge.numpy()
    for j in range(B):
        for k in range(int(cnt[j])):
            c = int(base[j]) + k
            L = np.log((pv[:, c, 1] * np.exp(pv[:, c, 0])).sum())
            assert abs(float(lse[j * beam + k]) - L) < 1e-12
            sc = s[c, :N].numpy().astype(np.float64)
            e = np.exp(sc - sc.max())
            for p in range(4):
                w, row = int(wl[4 * j + p]), 4 * j + p
                cw = e[words[:N, c] == w].sum() / e.sum()
                want = L + np.log((1 - lam) * np.exp(float(y[row, k]) - L) + lam * cw)
                assert abs(float(got[row, k]) - want) <= 2.0 ** -22 * (1 + abs(want)), (j, k, p)
        assert np.array_equal(got[4 * j:4 * j + 4, int(cnt[j]):], y[4 * j:4 * j + 4, int(cnt[j]):])      # slots past the count keep their bits
    assert float(lse[5]) == -7.0
    # a score that is not finite: the slot keeps its logits, bit 8; a finished sentence is skipped
    edge2 = torch.from_numpy(y.copy())
    s[1, 0] = float("inf")
    assert lib.jlm_memory_cell_patch(*args(edge=o(edge2), slen=o(_i32([4, 1])))) == 0 and int(flags[0]) == 8
    assert np.array_equal(edge2.numpy()[:4, 1], y[:4, 1]) and np.array_equal(edge2.numpy()[:4, 0], got[:4, 0])
    assert np.array_equal(edge2.numpy()[4:], y[4:])
    # the gather
    del lib.launches[:]
    H = 8
    pool = torch.from_numpy(rng.randn(10, H).astype(np.float32))
    out = torch.full((4, H), 9.0)
    rows, ndev = _i32([7, 2, 9, 0]), _i32([3])
    for bad in (dict(H=6), dict(H=0), dict(n=-1), dict(n=65536), dict(h=0), dict(rows=0), dict(out=0)):
        a = dict(dict(h=o(pool), H=H, pool=10, rows=o(rows), ndev=o(ndev), n=4, out=o(out), stream=0), **bad)
        assert lib.jlm_memory_gather_rows(*a.values()) == -1 and lib.launches == [], bad
    assert lib.jlm_memory_gather_rows(o(pool), H, 10, o(rows), o(ndev), 0, o(out), 0) == 0 and lib.launches == []
    assert lib.jlm_memory_gather_rows(o(pool), H, 10, o(rows), o(ndev), 4, o(out), 0) == 0 and lib.launches == ["memory_gather_rows"]
    assert torch.equal(out[:3], pool[[7, 2, 9]]) and bool((out[3] == 9.0).all())


# ---------------------------------------------------------------------------------------------- the decoders over the doubles
@pytest.fixture()
def decoder(monkeypatch):
    fake = fake_memory_edge.install(monkeypatch)
    cc.set_root("tied")
    from jlm_amd.decoder import Decoder
    d = Decoder(1)
    d.perf_timing = False
    d.fake = fake
    return d


def _memory(d, name="tied"):
    x, y = mc.streams(name)
    mem = M.Memory.build(d.model, x, y, 50)
    assert mem.N == len(mc.store(name)[0])
    return mem


def _check(got, want, n_q, tag):
    assert len(got) == len(want) and got[0][1] == want[0][1], (tag, got[0], want[0])
    for (g, gw), (w, _ww) in zip(got, want):
        assert abs(g - w) <= path_atol(True, 64, n_q, mc.THETA, len(gw)) + RTOL * abs(w), (tag, g, w)


def test_host_search_and_device_path_equal_the_proxy(decoder):
    """K >= N.  beam_width=None: the unpruned host-side search mixes every frame's probabilities by the float64 definition through the
    mixer plug; beam 5: the frame loop's double with the gather, the retrieval and the patch behind every frame's normaliser"""
    d, o = decoder, cc.oracle("tied")
    mem = _memory(d)
    mix = M.MemoryMix(mem, theta=mc.THETA, lam=mc.LAM, k=mc.K_ALL)
    pick = [i for i in range(len(SENTS)) if len(SENTS[i]) <= 4][:3]
    texts = [SENTS[i] for i in pick]
    plain = d.decode_batch(texts, beam_width=None)
    assert d.decode_batch(texts, beam_width=None, memory=None) == plain
    assert d.decode_batch(texts, beam_width=None, memory=M.MemoryMix(mem, theta=mc.THETA, lam=0.0, k=16)) == plain
    got = d.decode_batch(texts, beam_width=None, memory=mix)
    for text, g, p in zip(texts, got, plain):
        want, _sep = mc.memory_decode(o, text, None, "tied", mc.K_ALL, beam_width=None)
        assert [w for _, w in g] == [w for _, w in want]
        np.testing.assert_allclose([x for x, _ in g], [x for x, _ in want], rtol=2e-6, atol=2e-5)
        assert [x for x, _ in g] != [x for x, _ in p]
    # the device path
    moved = 0
    base = d.decode_batch(SENTS, beam_width=5)
    lists = d.decode_batch(SENTS, beam_width=5, memory=mix)
    for i, text in enumerate(SENTS):
        want, _sep = mc.memory_decode(o, text, None, "tied", mc.K_ALL, beam_width=5)
        _check(lists[i], want, mem.N, (i, text))
        moved += lists[i][0][1] != base[i][0][1]
    assert moved >= 4
    assert d.decode(SENTS[4], beam_width=5, memory=mix) == lists[4]
    # a sentence whose cells the device beam step cannot hold goes to the host with the beam, under the same mixture
    d.CAND_LIMIT = 5 * 3
    heavy = d.decode_batch(SENTS, beam_width=5, memory=mix)
    d.CAND_LIMIT = None
    assert any(h != l for h, l in zip(heavy, lists))                        # (some sentence took the host path: f64, other last bits)
    for i, text in enumerate(SENTS):
        want, _sep = mc.memory_decode(o, text, None, "tied", mc.K_ALL, beam_width=5)
        _check(heavy[i], want, mem.N, (i, text, "heavy"))


def test_launch_lists_with_and_without_a_memory(decoder):
    """memory=None and lam = 0 record exactly today's launch list; under a memory every stepped frame adds gather, retrieval, patch in
    front of the next beam step, and nothing else moves"""
    d = decoder
    mem = _memory(d)
    texts = SENTS[:5]
    d.fake.frame_log()
    plain = d.decode_batch(texts, beam_width=5)
    today = d.fake.frame_log()
    assert today and "memory_topk" not in today and today.count("beam_step") == max(len(t) for t in texts) + 1
    assert d.decode_batch(texts, beam_width=5, memory=None) == plain and d.fake.frame_log() == today
    assert d.decode_batch(texts, beam_width=5, memory=M.MemoryMix(mem, theta=mc.THETA, lam=0.0, k=16)) == plain
    assert d.fake.frame_log() == today
    mixed = d.decode_batch(texts, beam_width=5, memory=M.MemoryMix(mem, theta=mc.THETA, lam=mc.LAM, k=16))
    log = d.fake.frame_log()
    assert mixed != plain
    three = ["memory_gather_rows", "memory_topk", "memory_cell_patch"]
    assert [x for x in log if x not in three] == today
    at = [i for i, x in enumerate(log) if x == "memory_gather_rows"]
    assert len(at) == today.count("beam_step") - 1 and all(log[i:i + 4] == three + ["beam_step"] for i in at)
    # a batch without a memory behind one with: nothing is left on the plan
    assert d.decode_batch(texts, beam_width=5) == plain and d.fake.frame_log() == today


def test_refusals_before_anything_runs(decoder):
    d = decoder
    mem = _memory(d)
    mix = M.MemoryMix(mem, theta=mc.THETA, lam=mc.LAM, k=16)
    text = SENTS[1]
    from jlm_amd import context as jctx
    from jlm_amd.cache import CacheSpec
    from jlm_amd.ngram import NGramMix, NGramTable, pack
    spec = CacheSpec(16, theta=0.5, lam=0.5)
    ngram = NGramMix(NGramTable([pack([1])], [-1.0], [0.0], 1), 0.5)
    cached = object.__new__(jctx.CachedContext)
    other = types.SimpleNamespace(H=mem.H, split_lstm=mem.split, h_scale=mem.h_scale, V=mem.V)         # another model: the same shape is not enough
    foreign = M.MemoryMix(M.Memory(other, mem.keys, mem.words), k=16)
    d.model._primer = lambda: pytest.fail("primed")
    d._engine.submit = lambda *a, **k: pytest.fail("submitted")
    d.fake.frame_log()
    for call in (lambda: d.decode(text, context=[5, 6], cache=spec, memory=mix),
                 lambda: d.decode_batch([text], context=cached, memory=mix),
                 lambda: d.decode(text, ngram=ngram, memory=mix),
                 lambda: d.decode(text, vocab_select=True, memory=mix),
                 lambda: d.decode_predict(text, memory=mix),
                 lambda: d.decode_predict_batch([text], memory=mix),
                 lambda: d.decode_candidates(text, memory=mix),
                 lambda: d.decode_candidates_batch([text], memory=mix),
                 lambda: d.decode(text, memory=foreign),
                 lambda: d.decode(text, memory=mem),
                 lambda: d.decode(text, memory=0.5),
                 lambda: d.decode(text, beam_width=None, memory="mem.npz")):
        with pytest.raises(ValueError):
            call()
    # a device batch of more than 65 535 rows (the default max_batch keeps a chunk far below it)
    d.max_batch, d.plan_budget_bytes, keep = 4000, 1 << 40, (d.max_batch, d.plan_budget_bytes)
    assert len(d._chunks([text] * 4000, 17)[0]) * 17 > 65535
    with pytest.raises(ValueError, match="65535 rows"):
        d.decode_batch([text] * 4000, beam_width=17, memory=mix)
    d.max_batch, d.plan_budget_bytes = keep
    d.compat_quirks = True
    with pytest.raises(ValueError):
        d.decode(text, memory=mix)
    d.compat_quirks = False
    from jlm_amd import shard
    with pytest.raises(ValueError):
        shard.decode_sharded(d, [text], 0, 1, memory=mix)
    from jlm_amd.decoder_dynamic import DynamicDecoder
    dd = DynamicDecoder(1)
    with pytest.raises(ValueError):
        dd.decode(text, vocab_select=True, memory=mix)
    from jlm_amd.decoder_char import CharRNNDecoder
    from jlm_amd.decoder_ngram import NGramDecoder
    for cls in (CharRNNDecoder, NGramDecoder):
        with pytest.raises(ValueError):
            cls.decode(object.__new__(cls), text, memory=mix)
    # the engine refuses on its own too
    from jlm_amd.engine import DecodeEngine
    eng = object.__new__(DecodeEngine)
    eng.m, eng.torch = d.model.dev, None
    lat = types.SimpleNamespace(n_nodes=1, max_cands=1, n_sent=1, beam=5)
    for kw in (dict(vocab=(np.zeros(1), np.zeros(2)), memory=mix), dict(ngram=ngram, memory=mix), dict(memory=foreign),
               dict(memory=M.MemoryMix(mem, lam=0.0, k=16)), dict(kind="dynamic", dyn_lists=([], np.zeros(2, dtype=np.int64), [], [0]), memory=mix)):
        with pytest.raises(ValueError):
            DecodeEngine._submit(eng, lat, kw.pop("kind", "static"), kw.pop("vocab", None), kw.pop("dyn_lists", None), 10, False, **kw)
    with pytest.raises(ValueError):
        DecodeEngine._submit(eng, types.SimpleNamespace(n_nodes=1, max_cands=1, n_sent=4000, beam=17), "static", None, None, 10, False, memory=mix)
    assert d.fake.frame_log() == []                                         # nothing was launched


def test_a_plan_field_the_loop_refuses(decoder):
    """jlm_decode_frames' own refusals of the plan field come before its first launch: a memory beside a kind that is not 0, K out of
    range, a workspace below the retrieval's least"""
    import torch
    from jlm_amd import ops
    d = decoder
    mem = _memory(d)
    d.decode_batch(SENTS[:2], beam_width=5, memory=M.MemoryMix(mem, theta=mc.THETA, lam=mc.LAM, k=16))
    d.fake.frame_log()
    p = [q for q in d._engine.plans if q.memory_bufs is not None][0]
    mb, be = p.memory_bufs, ops.backend()
    seed = lambda **kw: be.seed_memory(p.obj, mem.keys, mem.words, mem.N, mem.H, mc.THETA, mc.LAM, kw.get("K", 16), mb.q_rows, mb.s,
                                       mb.ret_words, kw.get("workspace", mb.workspace), mb.flags)
    frames = lambda: be.decode_frames(d.model.dev.decode_model(), p.obj, 3, 0, 0, 0, False, False, 0)
    seed(workspace=torch.zeros(8))
    with pytest.raises(RuntimeError):
        frames()
    assert d.fake.frame_log() == [] and not p.obj.p.memory                  # refused before a launch; the op cleared the pointer
    seed()
    p.obj.p.kind = 1
    with pytest.raises(RuntimeError):
        frames()
    p.obj.p.kind = 0
    assert d.fake.frame_log() == []
    seed()
    be.clear_memory(p.obj)
    assert not p.obj.p.memory


# ---------------------------------------------------------------------------------------------- the command-line tools
def test_eval_flags_and_log_name():
    from jlm_amd import eval as jeval
    p = jeval.build_parser()
    a = p.parse_args([])
    assert not any(hasattr(a, k) for k in ("memory", "mem_theta", "mem_lam", "mem_k"))      # without the flag the namespace is what it was
    a = p.parse_args(["--memory", "mem.npz", "--mem-theta", "0.6", "--mem-lam", "0.5", "--mem-k", "16"])
    assert (a.memory, a.mem_theta, a.mem_lam, a.mem_k) == ("mem.npz", 0.6, 0.5, 16)
    ev = object.__new__(jeval.Evaluator)
    ev.args, ev.context_words, ev.cut_last, ev.cache = a, 0, 0, None
    plain = ev.log_name()                                                  # without the flag the name is what it was
    ev.memory_mix = None
    assert ev.log_name() == plain and "memory" not in plain
    ev.memory_mix = object()
    assert ev.log_name() == plain[:-len(".txt")] + "_memory.txt"
