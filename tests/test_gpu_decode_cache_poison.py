"""GPU: a decode under the continuous cache does not depend on what its buffers held before the call (tests/poison.py's fills):
the score scratch of the plan, and the slots of a ragged CachedContext below cap - count[r] -- zeroed memory that no kernel may
read.  The n-best must be equal bit for bit across the fills."""
import pytest

torch = pytest.importorskip("torch")
from jlm_amd.cache import CacheSpec                                      # noqa: E402
from tests import context_cases as cc                                    # noqa: E402
from tests import decode_cache_cases as dc                               # noqa: E402
from tests.poison import FILLS, bits, fill_tensor, first_difference      # noqa: E402
from tests.test_gpu_context import decoder                               # noqa: E402

pytestmark = pytest.mark.gpu

SENTS = cc.sentences()


@pytest.mark.parametrize("name", ["vtable", "tied-h512"])
def test_scratch_and_dead_slots_are_never_read(name):
    d, ctxs = decoder(name), dc.contexts(name)
    state = d.model.prime([cc.ids_of(c) for c in ctxs], cache=CacheSpec(16, theta=dc.THETA, lam=dc.LAM))
    assert len(set(state.count_host.tolist())) >= 3                       # a ragged batch: 0, a few, the full window
    clean = d.decode_batch(SENTS, beam_width=5, context=state)
    live = torch.arange(state.cap, device=state.words.device)[:, None] >= (state.cap - state.count.long())[None, :]
    for fill in FILLS:
        hist, words = state.hist.clone(), state.words.clone()
        fill_tensor(state.hist, fill)
        fill_tensor(state.words, fill)
        state.hist.copy_(torch.where(live[:, :, None], hist, state.hist))
        state.words.copy_(torch.where(live, words, state.words))
        filled = 0
        for p in d._engine.plans:
            bufs = getattr(p, "cache_bufs", None)
            if bufs is not None and not p.busy:
                fill_tensor(bufs.s, fill)
                filled += 1
        assert filled >= 1
        torch.cuda.synchronize()
        got = d.decode_batch(SENTS, beam_width=5, context=state)
        state.hist.copy_(hist)
        state.words.copy_(words)
        assert bits(got) == bits(clean), "the n-best depends on a buffer's earlier contents (fill %s): %s" % (
            fill.name, first_difference(got, clean))
