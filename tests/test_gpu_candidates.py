"""GPU: per-segment candidate lists end to end (Decoder.decode_candidates / decode_candidates_batch; csrc/jlm_alt.hip and
jlm_score_frames' launches behind jlm_decode_frames) against the UNMODIFIED oracle through tests/candidate_cases.py.

The five models of tests/context_cases.MODELS, its 12 inputs and one empty input, beams 1 / 5 / 17, with and without its contexts (as
word lists and as a primed ContextState, which must ``==`` each other), lookahead None / 0 / 1.  Bars: conversions ``==``
decode_batch's; the yardstick's spans and list lengths; scores within the suite's bar (rtol 2e-6 / atol 2e-5, below the 1.52e-4
separation tests/test_candidates_cpu.py measures for scores up to ~60; the fixtures' are below 40); the same word at every position but
those the yardstick alone leaves within 1e-4 of a neighbour at a finite lookahead (candidate_cases.EXPECTED_CLOSE names them: two
positions of one model, with contexts at lookahead 0; that there are no others, at most 2 per (model, beam), is asserted on the CPU); the own word's score within the bar of the path's."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
from tests import candidate_cases as kc                 # noqa: E402
from tests import context_cases as cc                   # noqa: E402
from tests import poison                                # noqa: E402

pytestmark = pytest.mark.gpu

TEXTS = kc.inputs()
_DEC = {}


def decoder(name):
    """the model's decoder, loaded once for the module"""
    if name not in _DEC:
        cc.set_root(name)
        from jlm_amd.decoder import Decoder
        _DEC[name] = Decoder(1)
    return _DEC[name]


@pytest.mark.parametrize("with_ctx", [False, True], ids=["plain", "context"])
@pytest.mark.parametrize("name", list(cc.MODELS))
def test_against_the_yardstick(name, with_ctx):
    d = decoder(name)
    ctxs = kc.contexts(cc.MODELS[name][0]) if with_ctx else None
    state = d.model.prime(ctxs) if with_ctx else None
    for beam in cc.BEAMS:
        conv = d.decode_batch(TEXTS, topN=kc.TOPN, beam_width=beam, context=ctxs)
        for la, rank in [(None, 0), (0, 0), (1, 0), (None, 1)]:
            got = d.decode_candidates_batch(TEXTS, topN=kc.TOPN, beam_width=beam, n_cand=kc.N_CAND, lookahead=la, rank=rank, context=ctxs)
            if with_ctx:
                assert got == d.decode_candidates_batch(TEXTS, topN=kc.TOPN, beam_width=beam, n_cand=kc.N_CAND, lookahead=la, rank=rank,
                                                        context=state), (name, beam, la, rank)
            assert [c for c, _s in got] == conv, (name, beam, la, rank)
            allowed = set(kc.close_positions(name, with_ctx, beam, la, rank))
            assert allowed <= kc.EXPECTED_CLOSE.get(name, set()) and (not allowed or la == 0), (name, beam, la, rank, allowed)
            for i, ((c, segs), (yc, lists)) in enumerate(zip(got, kc.yardstick(name, beam, with_ctx, la, rank))):
                if not len(TEXTS[i]):
                    assert (c, segs) == ([(0.0, [])], [])
                    continue
                cc.check_nbest(c, yc, (name, beam, i))
                if len(yc) <= rank:
                    assert segs == [], (name, beam, la, rank, i)
                    continue
                close = kc.check_segments(segs, lists, c, rank, (name, beam, with_ctx, la, rank, i))
                assert {(i, k, pos) for k, pos in close} <= allowed
            if beam == 1 and la is None and rank == 0:
                # a narrow beam is repaired: some alternative scores below the path the beam found (no echo of the n-best passes this)
                assert any(cands[0][0] < c[0][0] - 1e-4 for c, segs in got for _s, _l, cands in segs), name


@pytest.mark.parametrize("name", ["vtable", "tied-h512"])
def test_permuted_chunked_single_and_split_calls(name):
    d = decoder(name)
    ctxs = kc.contexts(cc.MODELS[name][0])
    ref = d.decode_candidates_batch(TEXTS, beam_width=5, context=ctxs)
    perm = list(np.random.RandomState(3).permutation(len(TEXTS)))
    got = d.decode_candidates_batch([TEXTS[i] for i in perm], beam_width=5, context=[ctxs[i] for i in perm])
    assert got == [ref[i] for i in perm]
    old = d.max_batch
    try:
        d.max_batch = 5                                          # three chunks
        assert d.decode_candidates_batch(TEXTS, beam_width=5, context=ctxs) == ref
    finally:
        d.max_batch = old
    for i in (0, 4, 7, 12):
        assert d.decode_candidates(TEXTS[i], beam_width=5, context=ctxs[i]) == ref[i], i
    widest = max(len(c) for _conv, segs in d.decode_candidates_batch(TEXTS, beam_width=5, n_cand=64, context=ctxs) for _s, _l, c in segs)
    assert widest >= 3
    try:
        d._engine.ALT_MAX_ROWS = widest - 1                      # a segment's alternatives fall into two device calls
        assert d.decode_candidates_batch(TEXTS, beam_width=5, context=ctxs) == ref
    finally:
        d._engine.ALT_MAX_ROWS = None
    assert not any(p.busy for p in d._engine.plans)


@pytest.mark.parametrize("name", ["tied", "untied"])
def test_results_do_not_depend_on_what_the_buffers_held(name):
    """the phase-2 row sets under both fills, and the decode's plans poisoned before the call"""
    d = decoder(name)
    for la in (None, 0):
        call = lambda: d.decode_candidates_batch(TEXTS, beam_width=5, lookahead=la)
        clean = poison.assert_same_three(call, what="candidate lists")
        for fill in poison.FILLS:
            for p in d._engine.plans:
                poison.poison_plan(p, fill)
            got = call()
            assert poison.bits(got) == poison.bits(clean), (fill.name, poison.first_difference(got, clean, "candidate lists"))


class _CountingOps:
    """the op backend with alt_frames' step counts written down"""

    def __init__(self, inner):
        self._inner, self.steps = inner, []

    def __getattr__(self, name):
        return getattr(self._inner, name)

    def alt_frames(self, *args):
        self.steps.append((int(args[-2]), list(args[21])))          # n_steps, n_live_host
        return self._inner.alt_frames(*args)


def test_lookahead_zero_enqueues_no_score_step(monkeypatch):
    from jlm_amd import ops
    d = decoder("tied")
    counting = _CountingOps(ops.backend())
    monkeypatch.setattr(ops, "_backend", counting)
    zero = d.decode_candidates_batch(TEXTS, beam_width=5, lookahead=0)
    assert counting.steps and all(s == 0 and not live for s, live in counting.steps)
    del counting.steps[:]
    full = d.decode_candidates_batch(TEXTS, beam_width=5)
    assert counting.steps and max(s for s, _live in counting.steps) >= 3
    # a path's last segment has nothing behind it: the same list at every lookahead
    for (_c, a), (_c2, b) in zip(zero, full):
        if a:
            assert a[-1] == b[-1]
