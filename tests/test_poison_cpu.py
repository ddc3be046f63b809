"""CPU: no result depends on what a buffer held before the call -- the helper of tests/poison.py against its own contract, and the
differential check of tests/test_gpu_poison.py through the numpy doubles of the C ABI (tests/fake_hip.py and its kin) at the smallest
shapes.  The same call runs with untouched allocations, with every ``torch.empty`` of jlm_amd/ filled with NaN / 0 / 0xFF (fill A) and
with 1e30 / 1 / 0x01 (fill B); results are equal bit for bit.  For the decode engine the buffers of a REUSED plan are filled between
two batches.  This keeps the doubles honest -- a double that swept dead rows would hide a kernel that does -- and lets the harness be
developed without a GPU.

Drivers without a double stay with the GPU module: score / score_streams without a cache (the cached op runs the same steps and is
covered here), complete / predict_top / predict_reading, decode(context=) and k-means."""
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")
from jlm_amd import config as jconfig, rowsets                                   # noqa: E402
from tests import context_cases as cc, fake_cache, fake_hip, fake_rank, fake_tail, poison            # noqa: E402
from tests import predict_cases as pc                                            # noqa: E402
from tests.gpu_rows import load_model, oracle_lm, ragged_prompts                # noqa: E402

RAGGED = (9, 1, 4, 7, 2, 7, 3)             # the live prefix shrinks at nearly every step


def _seqs(V, seed=3):
    rng = np.random.RandomState(seed)
    return [[int(w) for w in rng.randint(2, V, size=n)] for n in RAGGED]


# ---------------------------------------------------------------------------------------------------------------- the helper itself
def _fake_dev_model(H=8, ldt=12, V=10):
    return types.SimpleNamespace(torch=torch, device=torch.device("cpu"), H=H, ldt=ldt, V=V, mode="tied", split_lstm=False)


@pytest.mark.parametrize("fill", poison.FILLS, ids=lambda f: f.name)
def test_fill_by_dtype(fill):
    for dt in (torch.float64, torch.float32, torch.float16, torch.bfloat16):
        t = poison.fill_tensor(torch.zeros(5, dtype=dt), fill)
        if fill.name == "A":
            assert torch.isnan(t).all()
        else:
            assert torch.isfinite(t).all() and (t.double() >= min(1e30, float(torch.finfo(dt).max))).all()
    assert poison.fill_tensor(torch.zeros(3, dtype=torch.float32), poison.FILL_B).tolist() == [np.float32(1e30)] * 3
    for dt in (torch.int32, torch.int64, torch.int16):
        assert poison.fill_tensor(torch.full((4,), 7, dtype=dt), fill).tolist() == [fill.integer] * 4
    assert poison.fill_tensor(torch.zeros(4, dtype=torch.uint8), fill).tolist() == [fill.byte] * 4
    for shape in ((0,), (0, 7), (3, 0)):                                         # zero-sized: nothing to fill, nothing raised
        assert poison.fill_tensor(torch.empty(shape), fill).shape == shape
    # the fills themselves: in-range integers, never an extreme
    assert 0 <= fill.integer <= 1 and 0 < fill.byte <= 0xFF


@pytest.mark.parametrize("fill", poison.FILLS, ids=lambda f: f.name)
def test_only_callers_inside_the_package_are_poisoned(fill):
    empty, empty_like = torch.empty, torch.empty_like
    with poison.poisoned_allocations(fill) as rec:
        assert torch.empty is not empty and torch.empty.__wrapped__ is empty
        # this module, and torch's own code called from it (a Linear's parameters are torch.empty inside torch/nn)
        mine = torch.empty(6)
        torch.empty_like(mine)
        torch.nn.Linear(3, 2)
        assert rec.count == 0 and not rec.sites
        rs = rowsets.RowSets(_fake_dev_model(), 5, logits=True)               # rowsets.py's ``e = lambda ...``: the lambda's line
        assert rec.count == 6 and len(rec.sites) == 1
        (site,) = rec.sites
        assert site.startswith("jlm_amd/rowsets.py:") and site in poison.allocation_sites()
        want = np.float32(fill.floating)
        for t in rs.h + rs.c + [rs.T, rs.logits]:
            a = t.numpy()
            assert a.dtype == np.float32 and (np.isnan(a).all() if fill.name == "A" else (a == want).all())
        assert rs.logits.shape == (5, 12) and rs.T.shape == (5, 12)
        assert rs.flags.tolist() == [0] and rs.rows.tolist() == list(range(5))                 # zeros and arange stay what they are
        # a zero-sized tensor and a page-locked block from inside the package (lattice.StagingPool; pinning needs a device)
        from jlm_amd.lattice import StagingPool
        pool = StagingPool(torch, torch.cuda.is_available())
        blk = pool.get(24)
        assert blk.tensor.dtype == torch.int32 and blk.tensor.numel() >= 24 and (blk.tensor == fill.integer).all()
        assert blk.tensor.is_pinned() == torch.cuda.is_available()
        assert rowsets.RowSets(_fake_dev_model(), 0).h[0].shape == (0, 8)
    assert torch.empty is empty and torch.empty_like is empty_like
    assert rec.sites <= poison.allocation_sites()


def test_originals_return_after_an_exception():
    empty, empty_like, new_empty = torch.empty, torch.empty_like, torch.Tensor.new_empty
    with pytest.raises(RuntimeError, match="inside"):
        with poison.poisoned_allocations(poison.FILL_A):
            assert torch.empty is not empty
            raise RuntimeError("inside")
    assert torch.empty is empty and torch.empty_like is empty_like and torch.Tensor.new_empty is new_empty


def test_allocation_sites_are_the_packages_own():
    sites = poison.allocation_sites()
    assert sites and all(s.startswith("jlm_amd/") and int(s.rsplit(":", 1)[1]) > 0 for s in sites)
    for name in ("rowsets", "score", "cache", "complete", "compress", "model", "decoder_char", "engine", "lattice"):
        assert any(s.startswith("jlm_amd/%s.py:" % name) for s in sites), name
    # every buffer name of the plan lists is an attribute _Plan sets, and the lists do not overlap
    import inspect
    from jlm_amd import engine
    src = inspect.getsource(engine._Plan.__init__)
    names = poison.PLAN_DEVICE + poison.PLAN_PINNED + poison.PLAN_EXCLUDED
    assert len(set(names)) == len(names)
    for n in names:
        assert "self.%s" % n in src, n


def test_bits_is_bit_for_bit():
    nan = np.array([np.nan, 0.0])
    assert poison.bits(nan) == poison.bits(nan.copy()) and poison.bits(np.array([0.0])) != poison.bits(np.array([-0.0]))
    assert poison.bits([(1.5, ["a"])]) == poison.bits([(1.5, ["a"])]) and poison.bits([(1.5, ["a"])]) != poison.bits([(1.5, ["b"])])
    assert poison.bits(torch.tensor([1.0, float("nan")])) == poison.bits(torch.tensor([1.0, float("nan")]))
    assert "[1]" in poison.first_difference([np.zeros(3), np.array([1.0, 2.0])], [np.zeros(3), np.array([1.0, 3.0])])
    assert poison.first_difference({"a": 1.0}, {"a": 1.0}) is None


# ------------------------------------------------------------------------------------------------------- the row-set drivers' doubles
SITES = {}                                 # fill name -> the sites this module's differential cases reached
RAN = set()                                # the drivers whose cases ran
DRIVERS = {"rank", "cached", "generate", "predict", "decode", "decode_predict", "char"}


def test_rank_and_carried_state(monkeypatch):
    RAN.add("rank")
    fake_rank.install(monkeypatch)
    cc.set_root("vtable")
    from jlm_amd.model import LSTM_Model
    m = LSTM_Model(experiment_id=1)
    V = cc.MODELS["vtable"][0]
    seqs = _seqs(V)
    poison.assert_same_three(lambda: m.rank(seqs, cc.EOS, readings=True, max_prefix=3), SITES, "rank")
    x = np.random.RandomState(5).randint(0, V, size=(5, 9)).astype(np.int32)

    def streams():
        a, h, c = m.rank_streams(x[:, :4], x[:, 1:5])
        b, h2, c2 = m.rank_streams(x[:, 4:8], x[:, 5:9], h=h, c=c)
        return a, b, h2, c2
    poison.assert_same_three(streams, SITES, "rank_streams")


@pytest.mark.parametrize("name", ["tied", "untied"])
def test_cached_score_and_carried_cache(name, monkeypatch):
    """the cached op runs score_frames' steps: this is the CPU's score / score_streams too"""
    RAN.add("cached")
    from jlm_amd import cache as C
    fake_cache.install(monkeypatch)
    cc.set_root(name)
    from jlm_amd.model import LSTM_Model
    m = LSTM_Model(experiment_id=1)
    V = cc.MODELS[name][0]
    rng = np.random.RandomState(2)
    words = rng.randint(2, V, size=5)                                       # few words: matches and misses both
    seqs = [[int(w) for w in words[rng.randint(0, 5, size=n)]] for n in RAGGED]
    spec = C.CacheSpec(4, theta=[0.0, 0.7], lam=0.25)                       # a window shorter than the call
    poison.assert_same_three(lambda: m.score_cached(seqs, cc.EOS, spec), SITES, "score_cached")
    s = words[rng.randint(0, 5, size=(3, 13))].astype(np.int32)

    def streams():
        a = m.score_streams_cached(s[:, :7], s[:, 1:8], spec)
        b = m.score_streams_cached(s[:, 7:12], s[:, 8:13], spec, a.h, a.c, a.state)
        return [(r.nll_lm, r.logp_cache, r.n_entries, r.h, r.c, r.state.numpy()) for r in (a, b)]
    poison.assert_same_three(streams, SITES, "score_streams_cached")


def test_generate_plain_and_truncated(fx, monkeypatch):
    RAN.add("generate")
    from jlm_amd import ops as _ops
    from tests.test_generate_truncated_cpu import OracleOps
    f = fx("small-vtable")
    fake = fake_hip.install(monkeypatch)
    monkeypatch.setattr(_ops, "_backend", OracleOps(fake, oracle_lm(f["root"])))
    model = load_model(f["root"])
    prompts = ragged_prompts(7, model.dev.V, seed=4)
    for kw in (dict(temperature=0.0), dict(temperature=1.0, stop_id=1), dict(temperature=0.9, top_k=5), dict(temperature=1.1, top_p=0.6)):
        poison.assert_same_three(lambda: model.generate(prompts, 4, seed=11, **kw), SITES, "generate %r" % (kw,))


@pytest.mark.parametrize("name", ["small-tied", "small-untied", "small-vtable", "small-tied-sn"])
def test_predict_and_project(name, fx, monkeypatch):
    """the model.py sites: predict (the step's outputs, T, the logits and their softmax) and project"""
    RAN.add("predict")
    fake_hip.install(monkeypatch)
    f = fx(name)
    model = load_model(f["root"])
    rng = np.random.RandomState(1)
    hid = rng.randn(5, model.hidden_size) * 0.3

    def call():
        model.hidden, model.cell = hid.copy(), hid[::-1].copy()
        out = [model.predict([3, 7, 11, 2, 1999])[:2]]
        out.append(model.predict([5, 6, 7, 8, 9])[:2] + (model.hidden, model.cell))
        out.append(model.project(hid))
        if f["cfg"]["share_embedding"]:
            out.append(model.predict([1, 2, 3, 4, 5], vocab=[7, 1500, 3, 600, 1999])[:2])      # five columns: three of padding
        return out
    poison.assert_same_three(call, SITES, "predict / project")


# ---------------------------------------------------------------------------------------------------------------- the decode engine
def _decoder_factory(root, kind):
    def make():
        jconfig.set_root(root)
        from jlm_amd.decoder import Decoder
        from jlm_amd.decoder_dynamic import DynamicDecoder
        d = (DynamicDecoder if kind == "dynamic" else Decoder)(1)
        d.perf_timing = False
        return d
    return make


# (top_sampling: the 150 most frequent words join every sentence's list -- a plan's key holds the size class of the batch's longest list,
#  engine._submit, and both batches must meet the same plan)
SELECT = {"vocab_select": True, "samples": 150, "top_sampling": True}


# (the double gathers whole candidate blocks of T and the beam's rows before it masks them: under a fill numpy warns about the
#  stale values' casts, and the results show that none of them is used)
@pytest.mark.filterwarnings("ignore:invalid value encountered:RuntimeWarning", "ignore:overflow encountered:RuntimeWarning")
@pytest.mark.parametrize("kind,kw", [("static", {}), ("static", SELECT), ("dynamic", SELECT)], ids=["static", "vocab-select", "dynamic"])
@pytest.mark.parametrize("name", ["small-tied", "small-vtable"])
def test_reused_plan(name, kind, kw, fx, monkeypatch):
    RAN.add("decode")
    fake_hip.install(monkeypatch)
    f = fx(name)
    dirty = poison.kana_sentences(poison.DIRTY_LENGTHS, 31, f["alphabet"])
    target = poison.kana_sentences(poison.TARGET_LENGTHS, 32, f["alphabet"])
    call = lambda dec, sents: dec.decode_batch(sents, beam_width=poison.REUSE_BEAM, **kw)
    make = _decoder_factory(f["root"], kind)
    poison.assert_reuse(make(), make(), call, dirty, target, "%s %s" % (name, kind))
    # ... and the allocations of a batch's own (the plan, the lattice's staging block)
    poison.assert_same_three(lambda: call(make(), target), SITES, "%s %s on a new plan" % (name, kind))


def test_reused_plan_predicting_the_last_word(monkeypatch):
    RAN.add("decode_predict")
    fake_tail.install(monkeypatch)

    def make():
        cc.set_root("tied")
        from jlm_amd.decoder import Decoder
        d = Decoder(1)
        d.perf_timing = False
        return d
    dirty = poison.kana_sentences(poison.DIRTY_LENGTHS, 33, cc.ALPHABET)
    target = poison.kana_sentences(poison.TARGET_LENGTHS, 34, cc.ALPHABET)
    call = lambda dec, sents: dec.decode_predict_batch(sents, topN=pc.TOPN, beam_width=poison.REUSE_BEAM)
    poison.assert_reuse(make(), make(), call, dirty, target, "decode_predict")
    poison.assert_same_three(lambda: call(make(), target), SITES, "decode_predict on a new plan")


def test_character_decoder(fx, monkeypatch):
    RAN.add("char")
    fake_hip.install(monkeypatch)
    f = fx("small-char")

    def make():
        jconfig.set_root(f["root"])
        from jlm_amd.decoder_char import CharRNNDecoder
        return CharRNNDecoder(1)
    dirty = poison.kana_sentences(poison.DIRTY_LENGTHS, 35, f["alphabet"])
    target = poison.kana_sentences(poison.TARGET_LENGTHS, 36, f["alphabet"])
    dec = make()
    dec.decode_batch(dirty, beam_width=poison.REUSE_BEAM)                  # the same decoder after a longer batch
    poison.assert_same_three(lambda: dec.decode_batch(target, beam_width=poison.REUSE_BEAM), SITES, "character decoder")
    assert poison.bits(dec.decode_batch(target, beam_width=poison.REUSE_BEAM)) == \
        poison.bits(make().decode_batch(target, beam_width=poison.REUSE_BEAM))


def test_sites_reached_on_the_cpu():
    """Runs last: what the cases above reached under each fill.  Every site but those of the drivers that have no double (this
    module's docstring) -- the closure over ALL sites is the GPU module's."""
    for fill in poison.FILLS:
        assert SITES.get(fill.name, set()) <= poison.allocation_sites()
    if RAN != DRIVERS:                 # a selection of this module's tests (-k): nothing more to say
        return
    no_double = ("jlm_amd/complete.py", "jlm_amd/compress.py")
    want = {s for s in poison.allocation_sites() if not s.startswith(no_double)}
    for fill in poison.FILLS:
        missing = want - SITES[fill.name]
        assert not missing, (fill.name, sorted(missing))
