"""CPU: the chunk pipeline under Decoder.decode_batch, Decoder.decode_predict_batch and DynamicDecoder.decode_batch over the numpy double
(tests/fake_hip.py, tests/fake_tail.py) -- a failure in the middle of a multi-chunk call leaves no batch uncollected and no plan busy,
and decode_predict_batch hands the engine the chunks decode_batch does."""
import numpy as np
import pytest

from jlm_amd import context as jctx
from jlm_amd.engine import Ticket
from tests import context_cases as cc
from tests import fake_tail

INPUTS = [s[:4] for s in cc.sentences()[:5]]              # five short inputs: three chunks at max_batch = 2
CALLS = {
    "decode_batch": (False, lambda d, **kw: d.decode_batch(INPUTS, beam_width=3, **kw)),
    "decode_predict_batch": (False, lambda d, **kw: d.decode_predict_batch(INPUTS, topN=3, beam_width=3, **kw)),
    "dynamic": (True, lambda d, **kw: d.decode_batch(INPUTS, beam_width=3, vocab_select=True, **kw)),
}


def _decoder(dynamic, monkeypatch):
    fake_tail.install(monkeypatch)
    cc.set_root("tied")
    from jlm_amd.decoder import Decoder
    from jlm_amd.decoder_dynamic import DynamicDecoder
    d = (DynamicDecoder if dynamic else Decoder)(1)
    d.perf_timing = False
    d.max_batch = 2
    assert len(d._chunks(INPUTS, 3)) >= 3
    return d


@pytest.mark.parametrize("entry", list(CALLS))
def test_failure_mid_pipeline_collects_every_batch(entry, monkeypatch):
    """the second collect of a call of three chunks raises: the exception reaches the caller, every ticket the engine handed out was
    collected (the failing one included: once), and no plan is left busy"""
    dynamic, call = CALLS[entry]
    d = _decoder(dynamic, monkeypatch)
    eng = d._engine
    want = call(d)
    submit, collect = eng.submit, eng.collect
    submitted, collected = [], []

    def submit_(*a, **kw):
        submitted.append(submit(*a, **kw))
        return submitted[-1]

    def collect_(ticket):
        collected.append(ticket)
        out = collect(ticket)                                # (a collect that fails releases its plan first, as the engine's own do)
        if len(collected) == 2:
            raise RuntimeError("the second collect")
        return out

    monkeypatch.setattr(eng, "submit", submit_)
    monkeypatch.setattr(eng, "collect", collect_)
    with pytest.raises(RuntimeError, match="the second collect"):
        call(d)
    assert len(submitted) >= 2 and len(collected) == len(submitted)
    assert all(any(t is s for t in collected) for s in submitted)
    assert not any(p.busy for p in eng.plans)
    assert not eng.pipelined
    monkeypatch.setattr(eng, "submit", submit)
    monkeypatch.setattr(eng, "collect", collect)
    assert call(d) == want                                   # and the decoder is as usable as before


def test_predict_hands_the_engine_the_chunks_of_decode_batch(monkeypatch):
    """decode_predict_batch over non-empty inputs: per submit the same sentences and the same context rows as decode_batch over the same
    inputs and contexts ("the same chunks: the same bits"), with the state's rows in another order than the inputs"""
    d = _decoder(False, monkeypatch)
    n = len(INPUTS)
    assert len(set(INPUTS)) == n
    state = jctx.ContextState(d.model.dev, None, None, None, None, np.arange(2, 2 + n), np.ones(n))
    rows = [3, 0, 4, 1, 2]
    log = []

    def submit(lat, kind, context=None, **kw):
        log.append(([INPUTS.index(t) for t in lat.texts], context[0], list(context[1]), kind))
        return Ticket(None, lat, kw["topN"], kw["timing"], None, None)

    monkeypatch.setattr(d._engine, "submit", submit)
    monkeypatch.setattr(d._engine, "collect", lambda ticket: [(None, None)] * ticket.lat.n_sent)
    d.decode_batch(INPUTS, topN=3, beam_width=3, context=jctx.DecodeContext(state, rows))
    plain, log[:] = list(log), []
    d.decode_predict_batch(INPUTS, topN=3, beam_width=3, context=jctx.DecodeContext(state, rows))
    assert len(plain) >= 3 and log == plain
    assert sorted(i for idx, *_ in plain for i in idx) == list(range(n))
    for idx, st, r, kind in plain:
        assert st is state and r == [rows[i] for i in idx] and kind == "static"
