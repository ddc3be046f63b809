"""Control over what an uninitialised buffer holds (tests/test_poison_cpu.py, tests/test_gpu_poison.py).

The drivers of jlm_amd hand their kernels ``torch.empty`` memory, and a decode plan (jlm_amd/engine.py ``_Plan``) is reused by every
later batch of its shape.  A kernel that reads a row, a padding column or a partial that its call never wrote looks right as long as
that memory holds zeros or the previous call's correct values.  Here that memory is filled on purpose:

  fill   floating point   int32 / int64   uint8
  A      NaN              0               0xFF
  B      +1e30            1               0x01

NaN alone is not enough: a maximum and every ``>`` swallow a NaN, so a stale value read into a running maximum or a threshold test
shows only under the large finite fill.  The integer fills are small in-range values on purpose: most integer buffers are indices, and
a stale read must show up as a different answer, never as a wild access.

:func:`poisoned_allocations` patches the allocators for callers inside ``jlm_amd/`` only; :func:`poison_plan` fills the buffers of a
decode plan; :func:`allocation_sites` lists the sites the package has, for the closure check of the GPU module.
"""
import contextlib
import os
import re
import sys
from collections import namedtuple

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "jlm_amd") + os.sep

Fill = namedtuple("Fill", "name floating integer byte")
FILL_A = Fill("A", float("nan"), 0, 0xFF)
FILL_B = Fill("B", 1e30, 1, 0x01)
FILLS = (FILL_A, FILL_B)

_SITE = re.compile(r"torch\.empty\(|empty_like\(|new_empty\(")


def allocation_sites():
    """the ``file:line`` (file relative to the repository) of every ``torch.empty(``, ``empty_like(`` and ``new_empty(`` in
    jlm_amd/*.py; a line with several calls is one site"""
    sites = set()
    for name in sorted(os.listdir(PKG)):
        if not name.endswith(".py"):
            continue
        with open(os.path.join(PKG, name), encoding="utf-8") as f:
            for no, line in enumerate(f, 1):
                code = line.split("#", 1)[0]
                if _SITE.search(code):
                    sites.add("jlm_amd/%s:%d" % (name, no))
    return sites


def uses_new_empty():
    for name in os.listdir(PKG):
        if name.endswith(".py"):
            with open(os.path.join(PKG, name), encoding="utf-8") as f:
                if "new_empty(" in f.read():
                    return True
    return False


def fill_tensor(t, fill):
    """``t`` filled by its dtype, in place, on its own device and the current stream (a zero-sized tensor: nothing to do)"""
    import torch
    if t.numel() == 0:
        return t
    if t.dtype.is_floating_point:
        v = fill.floating
        if v == v and abs(v) > torch.finfo(t.dtype).max:          # 1e30 in a half: the largest finite value instead of inf
            v = torch.finfo(t.dtype).max
        t.fill_(v)
    elif t.dtype == torch.uint8:
        t.fill_(fill.byte)
    elif t.dtype == torch.bool:
        t.fill_(bool(fill.integer))
    elif t.dtype.is_complex:
        t.fill_(complex(fill.floating, fill.floating))
    else:
        t.fill_(fill.integer)
    return t


def _caller_site(depth=2):
    """``file:line`` of the nearest caller frame outside torch when that frame lies in jlm_amd/, else None"""
    import torch
    torch_dir = os.path.dirname(os.path.abspath(torch.__file__)) + os.sep
    f = sys._getframe(depth)
    while f is not None:
        path = os.path.abspath(f.f_code.co_filename)
        if not path.startswith(torch_dir):
            if path.startswith(PKG):
                return "%s:%d" % (os.path.relpath(path, REPO).replace(os.sep, "/"), f.f_lineno)
            return None
        f = f.f_back
    return None


class Recorder:
    """what a :func:`poisoned_allocations` block saw: ``sites`` the call sites filled, ``count`` the tensors"""

    def __init__(self, fill):
        self.fill, self.sites, self.count = fill, set(), 0


@contextlib.contextmanager
def poisoned_allocations(fill, record=None):
    """Inside the block ``torch.empty`` and ``torch.empty_like`` (and ``Tensor.new_empty`` when jlm_amd/ calls it) return tensors
    filled with ``fill`` when the nearest caller frame outside torch lies in jlm_amd/; every other caller gets the original function's
    result untouched.  Yields a :class:`Recorder`; ``record``: a set that also receives the sites (shared across blocks).  The
    originals are back on exit, also after an exception.  Not reentrant, and process-wide: other threads allocating from jlm_amd/
    meanwhile are poisoned too (the decoders' lattice workers: that is wanted)."""
    import torch
    rec = Recorder(fill)
    originals = [(torch, "empty", torch.empty), (torch, "empty_like", torch.empty_like)]
    if uses_new_empty():
        originals.append((torch.Tensor, "new_empty", torch.Tensor.new_empty))

    def wrap(orig):
        def patched(*args, **kwargs):
            t = orig(*args, **kwargs)
            site = _caller_site()
            if site is not None:
                fill_tensor(t, fill)
                rec.sites.add(site)
                rec.count += 1
                if record is not None:
                    record.add(site)
            return t
        patched.__wrapped__ = orig
        return patched

    try:
        for owner, name, orig in originals:
            setattr(owner, name, wrap(orig))
        yield rec
    finally:
        for owner, name, orig in originals:
            setattr(owner, name, orig)


# --------------------------------------------------------------------------------------------------------------------- decode plans
# device buffers a batch must write before it reads ...
PLAN_WRITE_FIRST = ("score", "lse", "ysum", "bp", "node", "word", "live", "edge", "h", "c", "T", "run_max", "run_sum", "part",
                    "out_nodes", "out_score", "pr_score", "pr_row", "pr_word", "pr_len", "pr_nodes")
# ... and those zeroed once at construction, which hold another batch's values after any reuse anyway
PLAN_ZEROED_ONCE = ("cnt", "n_live", "live_base", "Tm", "out_len")
PLAN_DEVICE = PLAN_WRITE_FIRST + PLAN_ZEROED_ONCE
# page-locked read-back blocks (h_len is torch.zeros at construction and copied whole from out_len by every batch, like the others)
PLAN_PINNED = ("h_nodes", "h_len", "h_score", "h_nlive", "h_pr_score", "h_pr_row", "h_pr_word", "h_pr_len", "h_pr_nodes")
# inputs of the batch: the staged lattice and the constant index arrays, the left context, the spans of a predicted last word
PLAN_EXCLUDED = ("dev_ints", "host_ints", "ctx_prev", "ctx_word", "ctx_idx", "ctx_idx_host", "pr_ints", "pr_host")


def plan_tensors(plan):
    """{attribute: tensor} of every torch tensor attribute of ``plan``"""
    import torch
    return {k: v for k, v in vars(plan).items() if isinstance(v, torch.Tensor)}


def poison_plan(plan, fill):
    """Every buffer of PLAN_DEVICE and PLAN_PINNED that ``plan`` has, filled with ``fill``; the device synchronised afterwards.
    AssertionError for a busy plan (a batch in flight owns its buffers).  -> the names filled"""
    import torch
    assert not plan.busy, "the plan is in flight"
    done = []
    for name in PLAN_DEVICE + PLAN_PINNED:
        t = getattr(plan, name, None)
        if t is None:
            continue
        fill_tensor(t, fill)
        done.append(name)
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    return done


def check_plan_closure(plan):
    """AssertionError unless every tensor attribute of ``plan``, on the device or page-locked, is in a fill list or the exclusion list"""
    known = set(PLAN_DEVICE) | set(PLAN_PINNED) | set(PLAN_EXCLUDED)
    missing = sorted(k for k in plan_tensors(plan) if k not in known)           # (the page-locked host blocks too)
    assert not missing, "decode-plan buffers neither poisoned nor excluded: %s" % missing


# ------------------------------------------------------------------------------------------------------------- the differential check
def bits(x):
    """``x`` -- arrays, tensors, floats, strings and containers of them -- as a value whose ``==`` is equality bit for bit: an array is
    (dtype, shape, bytes), so NaN equals NaN of the same bits and -0.0 differs from 0.0"""
    import numpy as np
    import torch
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().contiguous()
        return ("tensor", str(x.dtype), tuple(x.shape), x.view(torch.uint8).numpy().tobytes() if x.numel() else b"")
    if isinstance(x, np.ndarray):
        return ("array", str(x.dtype), x.shape, np.ascontiguousarray(x).tobytes())
    if isinstance(x, (float, np.floating)):
        return ("float", np.float64(x).tobytes())
    if isinstance(x, (bool, int, np.integer, str, bytes, type(None))):
        return x
    if isinstance(x, dict):
        return ("dict", tuple((k, bits(v)) for k, v in sorted(x.items())))
    if isinstance(x, (list, tuple)):
        return ("seq", tuple(bits(v) for v in x))
    raise TypeError("bits: %r" % type(x))


def first_difference(a, b, path="result"):
    """where two results differ, for the assertion message: the path of the first differing leaf and the two values"""
    import numpy as np
    import torch
    a, b = (x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x for x in (a, b))
    if isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)):
        if len(a) != len(b):
            return "%s: lengths %d and %d" % (path, len(a), len(b))
        for i, (u, v) in enumerate(zip(a, b)):
            if bits(u) != bits(v):
                return first_difference(u, v, "%s[%d]" % (path, i))
        return None
    if isinstance(a, dict) and isinstance(b, dict):
        for k in sorted(set(a) | set(b)):
            if k not in a or k not in b or bits(a[k]) != bits(b[k]):
                return first_difference(a.get(k), b.get(k), "%s[%r]" % (path, k))
        return None
    if isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.shape == b.shape and a.dtype == b.dtype:
        raw = np.ascontiguousarray(a).view(np.uint8).reshape(a.shape + (-1,)) != np.ascontiguousarray(b).view(np.uint8).reshape(b.shape + (-1,))
        bad = np.argwhere(raw.any(axis=-1)) if a.size else []
        if len(bad):
            i = tuple(int(k) for k in bad[0])
            return "%s%s: %r against %r (%d of %d elements differ)" % (path, list(i), a[i], b[i], len(bad), a.size)
        return None
    if isinstance(a, np.ndarray) and isinstance(b, np.ndarray):
        return "%s: %s %s against %s %s" % (path, a.dtype, a.shape, b.dtype, b.shape)
    return None if bits(a) == bits(b) else "%s: %r against %r" % (path, a, b)


def run_three(call, record=None):
    """``call()`` with untouched allocations, under fill A and under fill B -> the three results; ``record``: {fill name: set of
    sites} that receives the sites each poisoned run filled.  An exception of a poisoned run -- a JlmHipError the clean run did not
    raise -- propagates."""
    out = [call()]
    for fill in FILLS:
        with poisoned_allocations(fill, None if record is None else record.setdefault(fill.name, set())):
            out.append(call())
    return out


def assert_same_three(call, record=None, what="result"):
    """the assertion shape of both modules: the three runs of :func:`run_three` are equal bit for bit.  -> the clean result"""
    clean, a, b = run_three(call, record)
    for fill, got in zip(FILLS, (a, b)):
        assert bits(got) == bits(clean), "%s depends on what an uninitialised buffer held (fill %s): %s" % (
            what, fill.name, first_difference(got, clean, what))
    return clean


def kana_sentences(lengths, seed, alphabet):
    """one random kana string per entry of ``lengths``, over the first ``alphabet`` kana (the lexicon's alphabet of a fixture)"""
    import numpy as np
    from jlm_amd import synth
    rng = np.random.RandomState(seed)
    return ["".join(synth.KANA[c] for c in rng.randint(0, alphabet, size=int(n))) for n in lengths]


# 16 frames both: a plan's frame count is the longest sentence's kana + 1 (the root's frame), rounded up to 8 (engine._plan_for), so
# 15 kana are the most that share a bucket with 12
DIRTY_LENGTHS = (13, 14, 15, 15, 13, 14, 15)
TARGET_LENGTHS = (1, 2, 4, 7, 9, 12, 5)
REUSE_BEAM = 6


def beam_state(plan, n_frames):
    """what a batch left in its plan: cnt [F, B] and, per cell, the score / bp / node rows below its cnt (the rows a later frame or
    the backtrace may read).  cnt covers every cell of the plan, the frames the batch did not run included: they must read 0."""
    import numpy as np
    B, beam, F, rmax = plan.B, plan.beam, plan.F, plan.rmax
    cnt = plan.cnt.cpu().numpy().reshape(F, B).copy()
    score, bp, node = (getattr(plan, k).cpu().numpy().reshape(F, B, beam) for k in ("score", "bp", "node"))
    keep = np.arange(beam)[None, None, :] < cnt[:, :, None]
    assert cnt.min() >= 0 and cnt.max() <= beam
    return dict(cnt=cnt, score=score[keep], bp=bp[keep], node=node[keep], n_frames=int(n_frames))


FILLED = set()                             # the plan buffers poison_plan met, for the closure check of the GPU module


def reuse_case(dec, call, dirty, target, fill):
    """The plan-reuse case of one decode kind and one fill on the decoder ``dec``, whose engine starts without plans:
    ``call(dec, dirty)``, every plan of the engine poisoned with ``fill``, ``call(dec, target)`` -- which must run on the SAME plan
    object.  -> (the target's result, the beam state it left)"""
    eng = dec._engine
    assert not any(p.busy for p in eng.plans)
    del eng.plans[:]
    call(dec, dirty)
    plans = list(eng.plans)
    assert len(plans) == 1, [p.key for p in plans]
    check_plan_closure(plans[0])
    filled = poison_plan(plans[0], fill)
    assert {"score", "bp", "node", "cnt", "h_nodes", "h_score"} <= set(filled)
    FILLED.update(filled)
    got = call(dec, target)
    assert len(eng.plans) == 1 and eng.plans[0] is plans[0] and eng.last_state is plans[0], [p.key for p in eng.plans]
    return got, beam_state(plans[0], max(len(s) for s in target) + 1)


def reuse_reference(fresh, call, target):
    """the same batch on a newly made decoder, on a plan made for it (a decoder's load-time calibration may have decoded and left
    plans: they go first) -> (result, beam state, the plan's key)"""
    assert not any(p.busy for p in fresh._engine.plans)
    del fresh._engine.plans[:]
    want = call(fresh, target)
    assert len(fresh._engine.plans) == 1
    plan = fresh._engine.last_state
    return want, beam_state(plan, max(len(s) for s in target) + 1), plan.key


def assert_reuse(dec, fresh, call, dirty, target, what):
    """both fills of :func:`reuse_case` on ``dec`` against :func:`reuse_reference` on ``fresh``: n-best (words, and scores with ==)
    and beam state equal bit for bit"""
    want, ws, key = reuse_reference(fresh, call, target)
    for fill in FILLS:
        got, gs = reuse_case(dec, call, dirty, target, fill)
        assert dec._engine.plans[0].key == key
        assert bits(got) == bits(want), "%s on a reused plan (fill %s): %s" % (what, fill.name, first_difference(got, want, "n-best"))
        assert bits(gs) == bits(ws), "%s: beam state on a reused plan (fill %s): %s" % (what, fill.name, first_difference(gs, ws, "state"))
