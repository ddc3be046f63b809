"""GPU: no result depends on what a buffer held before the call.

The drivers hand their kernels ``torch.empty`` memory (jlm_amd/rowsets.py RowSets, score.py, cache.py, complete.py, compress.py,
model.py, decoder_char.py) and a decode plan (jlm_amd/engine.py _Plan) is reused by every later batch of its shape.  Freshly mapped
device memory is mostly zeros and torch's caching allocator hands a repeated call the previous, correct values of the same call, so a
kernel that reads a row, a padding column or a partial that its call never wrote looks right in every other test.  Here that memory
is filled on purpose (tests/poison.py): NaN / 0 / 0xFF (fill A) and 1e30 / 1 / 0x01 (fill B -- a maximum or a ``>`` swallows a NaN).

One assertion shape everywhere: the same call with untouched allocations, under fill A and under fill B; every documented output
equal bit for bit -- the same kernels on the same operands -- and no JlmHipError in a poisoned run that the clean run does not raise
(it would propagate).  Ragged inputs: 37 rows (two 32-row blocks, the second partial) of 1 .. 9 words, so the live prefix shrinks
at nearly every step; 163 rows on the H = 512 model (one 160-row tile and three).

Plan reuse: a dirty batch of longer sentences first, then every buffer of the plan filled, then the target batch on the SAME plan
object, against a decoder that has decoded nothing else: n-best and the beam state below every cell's count.

The closure test at the end fails -- it does not skip -- when an allocation site of the package or a buffer of the plan was not
reached under both fills by this module's cases: a new ``torch.empty`` cannot enter the package untested."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
from jlm_amd import cache as C, compress, config as jconfig, rowsets, synth                # noqa: E402
from jlm_amd.score import sentence_arrays, plan_rows                                         # noqa: E402
from tests import context_cases as cc, poison                                                # noqa: E402
from tests.gpu_rows import UNTIED_F32, load_model, ragged_prompts                           # noqa: E402

pytestmark = pytest.mark.gpu

H512 = "tied-h512"                         # tests/context_cases.py: the LSTM step's kernels are other code at H = 512
MODELS = ["small-tied", "small-vtable", "small-tied-sn", "small-dsoftmax", "small-untied", UNTIED_F32, "odd-vtable", "wide-vtable", H512]
SITES = {}                                 # fill name -> the allocation sites this module's cases reached
_MODEL, _DEC = {}, {}
# site -> reason, for a site no case here can reach.  Expected to stay empty.
ALLOWED_SITES = {}


def set_root(name, fx):
    fixture = name.partition("@")[0]
    if fixture in cc.MODELS:
        cc.set_root(fixture)
        return cc.model_root(fixture)
    root = fx(fixture)["root"]
    jconfig.set_root(root)
    return root


def model(name, fx):
    """the model of ``name`` ("<fixture>@<precision>": loaded under JLM_PRECISION), loaded once for the module"""
    if name not in _MODEL:
        with pytest.MonkeyPatch.context() as mp:
            if "@" in name:
                mp.setenv("JLM_PRECISION", name.partition("@")[2])
            _MODEL[name] = load_model(set_root(name, fx))
        d = _MODEL[name].dev
        assert name != UNTIED_F32 or rowsets.t_is_state(d)
        assert name != "odd-vtable" or (d.V == 2003 and rowsets.ld_logits(d.V) == 2004)       # one padding column
        assert name != H512 or d.H == 512
    set_root(name, fx)
    return _MODEL[name]


def n_rows(name):
    return 163 if name == H512 else 37


def ragged_seqs(name, V, seed=3, pool=None):
    """n_rows sequences of 1 .. 9 words (every length present); ``pool``: drawn from that many distinct words"""
    rng = np.random.RandomState(seed)
    n = n_rows(name)
    lens = np.concatenate([np.arange(1, 10), rng.randint(1, 10, size=n - 9)])
    rng.shuffle(lens)
    words = rng.randint(2, V, size=pool) if pool else None
    return [[int(w) for w in (words[rng.randint(0, pool, size=L)] if pool else rng.randint(2, V, size=L))] for L in lens]


def same3(call, what):
    return poison.assert_same_three(call, SITES, what)


# ------------------------------------------------------------------------------------------------------------------- the helper
@pytest.mark.parametrize("fill", poison.FILLS, ids=lambda f: f.name)
def test_fills_on_the_device_and_in_page_locked_memory(fill):
    from jlm_amd.lattice import StagingPool
    m = type("M", (), dict(torch=torch, device=torch.device("cuda", 0), H=8, ldt=12, V=10, mode="tied", split_lstm=False))()
    side = torch.cuda.Stream()
    with poison.poisoned_allocations(fill) as rec:
        with torch.cuda.stream(side):          # the fill runs on the current stream: what the next launch on it reads is the fill
            rs = rowsets.RowSets(m, 5, logits=True)
            got = rs.logits.clone()
        side.synchronize()
        blk = StagingPool(torch, True).get(24)
        assert torch.empty(3, device="cuda").shape == (3,) and rec.count == 7          # this module's own call is not counted
    assert blk.tensor.is_pinned() and (blk.tensor == fill.integer).all()
    a = got.cpu().numpy()
    assert a.shape == (5, 12) and (np.isnan(a).all() if fill.name == "A" else (a == np.float32(1e30)).all())
    assert rec.sites <= poison.allocation_sites() and len(rec.sites) == 2


# ----------------------------------------------------------------------------------------------------------- the row-set drivers
@pytest.mark.parametrize("name", MODELS)
def test_score(name, fx):
    m = model(name, fx)
    seqs = ragged_seqs(name, m.dev.V)
    same3(lambda: m.score(seqs, 1), "score")
    same3(lambda: m.score(seqs, 1, per_token=False), "score per_token=False")
    same3(lambda: m.score(seqs, 1, max_rows=33), "score in calls of 33 rows")


@pytest.mark.parametrize("name", MODELS)
def test_score_streams_carried(name, fx):
    m = model(name, fx)
    B = n_rows(name)
    x = np.random.RandomState(2).randint(0, m.dev.V, size=(B, 11))

    def call():
        a, h, c = m.score_streams(x[:, :5], x[:, 1:6])
        b, h2, c2 = m.score_streams(x[:, 5:10], x[:, 6:11], h, c)
        return a, b, h, c, h2, c2
    same3(call, "score_streams")


@pytest.mark.parametrize("name", MODELS)
def test_scorer_run_returns_the_live_rows_state(name, fx):
    """The rows live at the LAST step hold their final state in the returned h, c; a row that stopped earlier is undefined there
    (Scorer.run's docstring, DESIGN.md "What a buffer must hold before a call") and is left out of the comparison."""
    m = model(name, fx)
    seqs = ragged_seqs(name, m.dev.V, seed=5)
    (ch,) = plan_rows([len(s) for s in seqs], 1 << 20)
    word, target = sentence_arrays([np.asarray(seqs[i]) for i in ch["idx"]], 1, ch["n_steps"])
    live = int(ch["n_live"][-1])
    assert 1 <= live < len(seqs) and ch["n_steps"] == 9

    def call():
        seq, tok, h, c = m._scorer().run(word, target, ch["n_live"])
        return seq, tok, h[:live], c[:live]
    same3(call, "Scorer.run")


GENERATE = [dict(temperature=0.0), dict(temperature=1.0), dict(temperature=1.0, stop_id=1), dict(temperature=0.0, stop_id=1),
            dict(temperature=0.9, top_k=5), dict(temperature=1.1, top_p=0.6, stop_id=1)]


@pytest.mark.parametrize("name", MODELS)
def test_generate(name, fx):
    m = model(name, fx)
    prompts = ragged_prompts(n_rows(name), m.dev.V, seed=4, lo=1, hi=9)
    for kw in GENERATE:
        same3(lambda: m.generate(prompts, 5, seed=11, **kw), "generate %r" % (kw,))


@pytest.mark.parametrize("name", MODELS)
def test_complete_and_masked_top_k(name, fx):
    m = model(name, fx)
    V = m.dev.V
    prompts = ragged_prompts(n_rows(name), V, seed=6, lo=1, hi=9)
    same3(lambda: m.complete(prompts, 3, beam_width=4), "complete")
    same3(lambda: m.complete(prompts, 3, beam_width=4, stop_id=1, n_best=2), "complete with stop_id")
    same3(lambda: m.predict_top(prompts, n=6), "predict_top")
    # the masked top-k: a set holding only the last word (V = 2 003: the one word of the partial last chunk), a small set across the
    # vocabulary, and the unrestricted row
    last, some = np.array([V - 1], dtype=np.int64), np.array([0, V // 4, V // 4 + 1, V - 2, V - 1], dtype=np.int64)
    allowed = [(last, None, some)[p % 3] for p in range(len(prompts))]
    top = same3(lambda: m.predict_top(prompts, n=6, allowed=allowed), "predict_top(allowed=)")
    assert top[0][0].tolist() == [V - 1] and len(top[1][0]) == 6
    same3(lambda: m.complete(prompts, 2, beam_width=4, first_allowed=allowed), "complete(first_allowed=)")
    if not m.config.get("char_rnn"):
        readings = [synth.KANA[p % 3] for p in range(len(prompts))]
        same3(lambda: m.predict_reading(prompts, readings, n=6), "predict_reading")


@pytest.mark.parametrize("name", MODELS)
def test_rank(name, fx):
    m = model(name, fx)
    seqs = ragged_seqs(name, m.dev.V, seed=7)
    same3(lambda: m.rank(seqs, 1, readings=True, max_prefix=3), "rank")
    x = np.random.RandomState(8).randint(0, m.dev.V, size=(n_rows(name), 9))

    def streams():
        a, h, c = m.rank_streams(x[:, :4], x[:, 1:5], max_prefix=2)
        b, h2, c2 = m.rank_streams(x[:, 4:8], x[:, 5:9], h=h, c=c, max_prefix=2)
        return a, b, h2, c2
    same3(streams, "rank_streams")


@pytest.mark.parametrize("name", MODELS)
def test_cached_score(name, fx):
    m = model(name, fx)
    V = m.dev.V
    spec = C.CacheSpec(4, theta=[0.0, 0.7], lam=0.25)                        # two thetas, a window shorter than the call
    seqs = ragged_seqs(name, V, seed=9, pool=5)                               # few distinct words: matches and misses both
    same3(lambda: m.score_cached(seqs, 1, spec), "score_cached")
    rng = np.random.RandomState(10)
    s = rng.randint(2, V, size=5)[rng.randint(0, 5, size=(n_rows(name), 13))]

    def streams():
        a = m.score_streams_cached(s[:, :7], s[:, 1:8], spec)
        b = m.score_streams_cached(s[:, 7:12], s[:, 8:13], spec, a.h, a.c, a.state)
        return [(r.nll_lm, r.logp_cache, r.n_entries, r.h, r.c, r.state.numpy()) for r in (a, b)]
    out = same3(streams, "score_streams_cached")
    assert np.isfinite(out[1][1]).any() and np.isinf(out[1][1]).any()


@pytest.mark.parametrize("name", MODELS)
def test_predict_step_resident_project(name, fx):
    """the model.py sites: the step's outputs, T, the padded logits and their softmax"""
    m = model(name, fx)
    V, H = m.dev.V, m.dev.H
    rng = np.random.RandomState(1)
    hid = rng.randn(5, H) * 0.3
    pool_h = torch.from_numpy((rng.randn(9, H) * 0.3).astype(np.float32)).cuda()
    pool_c = torch.from_numpy((rng.randn(9, H) * 0.3).astype(np.float32)).cuda()
    prev = torch.tensor([3, 0, 8, 3, 1], dtype=torch.int32, device="cuda")
    word = torch.tensor([2, V - 1, 5, 7, 1], dtype=torch.int32, device="cuda")

    def call():
        m.hidden, m.cell = hid.copy(), hid[::-1].copy()
        out = [m.predict([3, 7, 11, 2, V - 1])[:2]]
        out.append(m.predict([5, 6, 7, 8, 9])[:2] + (m.hidden, m.cell))
        out.append(m.project(hid))
        if m.config.get("share_embedding"):
            out.append(m.predict([1, 2, 3, 4, 5], vocab=[7, V // 2, 3, V // 3, V - 1])[:2])       # five columns, three of padding
        h_out, c_out = torch.zeros(5, H, device="cuda"), torch.zeros(5, H, device="cuda")
        pred, n_cols, _t = m.step_resident(pool_h, pool_c, prev, word, h_out, c_out)
        torch.cuda.synchronize()
        out.append((pred[:, :n_cols], n_cols, h_out, c_out))
        return out
    same3(call, "predict / step_resident / project")


@pytest.mark.parametrize("bit", [4, 8])
@pytest.mark.parametrize("n", [1025, 65537])
def test_kmeans(n, bit):
    """codes, codebook and n_iter: the launcher clears only a prefix of the scratch block"""
    x = (np.random.RandomState(n + bit).standard_t(3, size=n) * 0.1).astype(np.float32)

    def call():
        code, book, info = compress.kmeans_device(x, bit, seed=3)
        return code, book, info["n_iter"], info["constant"]
    out = same3(call, "kmeans_device")
    assert out[2] >= 1 and not out[3]


# ------------------------------------------------------------------------------------------------------------------ plan reuse
def decoder(name, kind, fx, new=False):
    """a decoder of ``name`` for ``kind`` ("static" | "dynamic" | "char"): one per module, or -- ``new`` -- one that has decoded
    nothing yet"""
    key = (name, kind)
    if new or key not in _DEC:
        with pytest.MonkeyPatch.context() as mp:
            if "@" in name:
                mp.setenv("JLM_PRECISION", name.partition("@")[2])
            set_root(name, fx)
            from jlm_amd.decoder import Decoder
            from jlm_amd.decoder_char import CharRNNDecoder
            from jlm_amd.decoder_dynamic import DynamicDecoder
            d = dict(static=Decoder, dynamic=DynamicDecoder, char=CharRNNDecoder)[kind](1)
        d.perf_timing = False
        if new:
            return d
        _DEC[key] = d
    set_root(name, fx)
    return _DEC[key]


def alphabet_of(name, fx):
    return cc.ALPHABET if name in cc.MODELS else fx(name.partition("@")[0])["alphabet"]


# (top_sampling: the 150 most frequent words join every sentence's list -- a plan's key holds the size class of the batch's longest
#  list, engine._submit, and both batches must meet the same plan)
SELECT = dict(vocab_select=True, samples=150, top_sampling=True)
BEAM = poison.REUSE_BEAM


def _contexts(V):
    rng = np.random.RandomState(12)
    return [[], [int(rng.randint(2, V))], None] + [[int(w) for w in rng.randint(2, V, size=k)] for k in (3, 1, 6, 2)]


KINDS = {
    "static": ("static", lambda d, s, V: d.decode_batch(s, beam_width=BEAM)),
    "vocab-select": ("static", lambda d, s, V: d.decode_batch(s, beam_width=BEAM, **SELECT)),
    "dynamic": ("dynamic", lambda d, s, V: d.decode_batch(s, beam_width=BEAM, **SELECT)),
    "context": ("static", lambda d, s, V: d.decode_batch(s, beam_width=BEAM, context=_contexts(V))),
    "predict": ("static", lambda d, s, V: d.decode_predict_batch(s, topN=10, beam_width=BEAM)),
    "predict-context": ("static", lambda d, s, V: d.decode_predict_batch(s, topN=10, beam_width=BEAM, context=_contexts(V))),
}
REUSE = [("small-tied", "static"), ("small-tied-sn", "static"), ("small-untied", "static"), (UNTIED_F32, "static"),
         ("wide-vtable", "static"), (H512, "static"), ("small-tied", "vocab-select"), ("wide-vtable", "vocab-select"),
         ("small-tied", "dynamic"), ("small-vtable", "context"), (H512, "context"), ("small-tied", "dynamic-context"),
         ("small-vtable", "predict"), ("wide-vtable", "predict-context")]
KINDS["dynamic-context"] = ("dynamic", lambda d, s, V: d.decode_batch(s, beam_width=BEAM, context=_contexts(V), **SELECT))


def _timed(d, s):
    """the timed form of the frame loop (events around every kernel group, one stream): what bench.py's timed legs run"""
    d.perf_timing = True
    try:
        return d.decode_batch(s, beam_width=BEAM)
    finally:
        d.perf_timing = False
        del d.perf_log_lstm[:], d.perf_log_softmax[:]


# beyond the issue's list: the timed frame loop, a beam above one wave (the beam step's other form), and the flagship shape
# (V = 50 000, H = 512: every kernel at its production form)
KINDS["timed"] = ("static", lambda d, s, V: _timed(d, s))
KINDS["beam-70"] = ("static", lambda d, s, V: d.decode_batch(s, beam_width=70, topN=70))
REUSE += [("small-vtable", "timed"), ("small-tied", "beam-70"), ("mid-vtable", "static")]


@pytest.mark.parametrize("name,kind", REUSE, ids=["%s-%s" % r for r in REUSE])
def test_reused_plan(name, kind, fx):
    cls, run = KINDS[kind]
    dec = decoder(name, cls, fx)
    V = dec.model.dev.V
    call = lambda d, sents: run(d, sents, V)
    a = alphabet_of(name, fx)
    dirty = poison.kana_sentences(poison.DIRTY_LENGTHS, 31, a)
    target = poison.kana_sentences(poison.TARGET_LENGTHS, 32, a)
    fresh = decoder(name, cls, fx, new=True)
    poison.assert_reuse(dec, fresh, call, dirty, target, "%s %s" % (name, kind))
    assert name != "wide-vtable" or "Tm" in poison.FILLED

    # ... and a plan MADE under each fill (its torch.empty buffers and page-locked blocks, the lattice's staging block)
    def on_a_new_plan():
        del dec._engine.plans[:]
        if dec._engine.staging_pool is not None:
            dec._engine.staging_pool._free.clear()
        return call(dec, target)
    same3(on_a_new_plan, "%s %s on a new plan" % (name, kind))


@pytest.mark.parametrize("name,kind", [("small-vtable", "static"), ("small-tied", "dynamic")])
def test_reused_plans_of_a_pipelined_call(name, kind, fx):
    """chunks of three sentences: several plans in flight on the engine's streams, all of them poisoned between the two calls"""
    cls, run = KINDS[kind]
    a = alphabet_of(name, fx)
    dirty = poison.kana_sentences(poison.DIRTY_LENGTHS, 41, a)
    target = poison.kana_sentences((12, 11, 12, 9, 12, 10, 12), 42, a)          # every chunk in the dirty chunks' frame bucket
    fresh = decoder(name, cls, fx, new=True)
    fresh.max_batch = 3
    del fresh._engine.plans[:]
    want = run(fresh, target, fresh.model.dev.V)
    dec = decoder(name, cls, fx)
    old = dec.max_batch
    dec.max_batch = 3
    try:
        for fill in poison.FILLS:
            del dec._engine.plans[:]
            run(dec, dirty, dec.model.dev.V)
            plans = list(dec._engine.plans)
            assert len(plans) >= 2
            for p in plans:
                poison.poison_plan(p, fill)
            got = run(dec, target, dec.model.dev.V)
            assert {id(p) for p in dec._engine.plans} == {id(p) for p in plans}
            assert poison.bits(got) == poison.bits(want), (fill.name, poison.first_difference(got, want, "n-best"))
    finally:
        dec.max_batch = old
        del dec._engine.plans[:]


def test_character_decoder_lock_step_batch(fx):
    """no plan here: a state pool and per-frame torch.empty rows (decoder_char.py); the target batch after a longer one, the three
    runs, and a decoder that has decoded nothing else"""
    dec = decoder("small-char", "char", fx)
    a = alphabet_of("small-char", fx)
    dirty = poison.kana_sentences(poison.DIRTY_LENGTHS, 35, a)
    target = poison.kana_sentences(poison.TARGET_LENGTHS, 36, a)
    dec.decode_batch(dirty, beam_width=BEAM)
    got = same3(lambda: dec.decode_batch(target, beam_width=BEAM), "character decoder")
    fresh = decoder("small-char", "char", fx, new=True)
    assert poison.bits(got) == poison.bits(fresh.decode_batch(target, beam_width=BEAM))


# --------------------------------------------------------------------------------------------------------------------- closure
def test_every_site_and_every_plan_buffer_was_reached():
    """Runs last, after the whole module.  Fails when run alone: that is its point."""
    sites = poison.allocation_sites()
    assert set(ALLOWED_SITES) <= sites and all(ALLOWED_SITES.values())
    for fill in poison.FILLS:
        missing = sites - SITES.get(fill.name, set()) - set(ALLOWED_SITES)
        assert not missing, "allocation sites no case reached under fill %s: %s" % (fill.name, sorted(missing))
    # every name poison_plan fills was met on a plan (a renamed buffer would silently drop out of the fill); that no tensor of a plan
    # is outside the fill and exclusion lists was asserted on every plan the cases above reused (poison.check_plan_closure)
    unmet = set(poison.PLAN_DEVICE + poison.PLAN_PINNED) - poison.FILLED
    assert not unmet, "plan buffers poison_plan never met: %s" % sorted(unmet)
