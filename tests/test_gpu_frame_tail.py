"""GPU: the fused frame tail (jlm_pack_edge_mx6, csrc/jlm_frame_tail.hip) against the two launches it replaces.

Kernel level, through the C ABI on synthetic data: for the same T, lattice word lists and beam state
  (a) jlm_pack_t_mixed6 over the frame's live list + jlm_edge_logits       and       (b) jlm_pack_edge_mx6
must leave the SAME BYTES in the packed buffer and in edge[] -- both buffers are filled with a sentinel first and compared whole, so
every compact row below n_live, every edge entry written, and every byte (a) leaves untouched are covered.  The quantiser is one
__device__ function shared by both kernels (csrc/jlm_mx6_pack.h) and the dot products keep wordlist_kernel<0>'s order of operations, so
nothing less than equality is expected.

Decode level: the static golden cases on D-softmax* models through Decoder.decode_batch, default against JLM_FUSE_TAIL=0, each in a fresh
child process (the knob is read once per process)."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
from jlm_amd import _lib            # noqa: E402
from tests import golden_cases as gc  # noqa: E402
from tests.operand_cases import tie_rows  # noqa: E402

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0xA5

# 5 sentences of unequal length; frames 0 .. 3.  frame < len: the cell is live; frame == len: the sentence's FINAL cell (rows, but not in
# the live list: live_base is poisoned); frame > len: no rows.
LENS = [3, 1, 3, 2, 3]
N_FRAMES = 4
# starting words per (frame, sentence): the pass boundaries 0 / 1 / 32 / 33 / 64 / 65 on live cells, final cells with and without words
N_WORDS = [[33, 1, 32, 0, 65],
           [64, 7, 2, 40, 5],        # (1, 1): s = 1 is final here, with words; (1, 4): a live cell by length whose cnt is 0
           [3, 4, 66, 0, 31],        # (2, 3): final, without words
           [9, 0, 0, 6, 12]]         # frame 3: the final cells of the length-3 sentences (0, 2, 4), two with words
CNT_ZERO = (1, 4)
FEWER = {(0, 1), (1, 2), (2, 0)}    # cells with fewer live rows than the beam (where the beam allows it)


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    lib = _lib.lib()
    buf = ctypes.create_string_buffer(128)
    assert lib.jlm_device_arch(0, buf, 128) == 0
    assert buf.value.decode().startswith("gfx950"), buf.value
    return lib


def _st():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _problem(widths, beam):
    """one batch: the model's segments, T, the beam state of every frame and the lattice's word lists"""
    rng = np.random.default_rng(1000 * len(widths) + beam)
    B, F, n = len(LENS), N_FRAMES, len(widths)
    rmax = B * beam
    ldt = (sum(widths) + 3) // 4 * 4
    V = 67 * n
    bounds = [67 * i for i in range(n + 1)]
    keep = []
    segs, msegs = (_lib.Segment * n)(), (_lib.Segment * n)()
    ts = (ctypes.c_float * n)()
    off = 0
    for i, k in enumerate(widths):
        Bg = _dev((rng.standard_normal((bounds[i + 1] - bounds[i], k)) * 0.3).astype(np.float32))
        keep.append(Bg)
        nb = k // 32 if k % 32 == 0 else (k + 2 + 31) // 32
        segs[i] = _lib.Segment(bounds[i], bounds[i + 1], k, off, Bg.data_ptr(), k)
        msegs[i] = _lib.Segment(bounds[i], bounds[i + 1], k, off, Bg.data_ptr(), 32 * nb)        # (the packers read k, t_off and ldb only)
        ts[i] = 2.0 ** -4
        off += k
    b2 = (rng.standard_normal(V) * 0.5).astype(np.float32)
    T = (np.tanh(rng.standard_normal((F * rmax, ldt))) * rng.uniform(1e-3, 4.0, size=(F * rmax, 1))).astype(np.float32)
    T[1] = 0.0                                         # an all-zero row (scale bytes 0), a tiny one, one with zeros in it
    T[2] *= np.float32(2.0 ** -30)
    T[3, ::2] = 0.0
    # rows whose f32 product with the packer's multiplier f32(2^-4 log2 e) is an f16 rounding tie while the exact product is not
    # (tests/operand_cases.py tie_values): the fused tail and the two launches must stay on ONE rounding of the f16 plane
    tie_at = np.arange(0, F * rmax, 5)
    T[tie_at] = tie_rows(np.float32(np.float32(2.0 ** -4) * np.float32(1.4426950408889634)), len(tie_at), ldt)
    ncell = F * B
    cnt, live_base = np.zeros(ncell, np.int32), np.zeros(ncell, np.int32)
    g0 = (np.arange(F)[:, None] * rmax + np.arange(B)[None, :] * beam).astype(np.int32).reshape(-1)
    live = np.full(F * rmax, -1, np.int32)
    n_live = np.zeros(F, np.int32)
    tm_rows = ((rmax + 31) // 32 + 1) * 32              # one block of 32 rows more than any live list needs: the poisoned rows
    for f in range(F):
        order = list(rng.permutation(B))               # the order the sentences' beam steps took their place in the live list
        base = 0
        for s in order:
            c = f * B + s
            if f > LENS[s] or (f, s) == CNT_ZERO:
                continue
            k_rows = max(1, beam - 3) if (f, s) in FEWER else beam
            cnt[c] = k_rows
            if f < LENS[s]:
                live_base[c] = base
                live[f * rmax + base:f * rmax + base + k_rows] = g0[c] + np.arange(k_rows)
                base += k_rows
            else:                                      # final cell: a stale base that would land in the spare block if it were used
                live_base[c] = tm_rows - 32 + s
        n_live[f] = base
    wl, wl_out, offs = [], [], [0]
    for f in range(F):
        for s in range(B):
            nw = N_WORDS[f][s]
            w = rng.integers(0, V, size=nw)
            if nw >= n:
                w[:n] = [bounds[i] + i for i in range(n)]         # words from every segment in one cell
                w = rng.permutation(w)
            wl += [int(x) for x in w]
            offs.append(len(wl))
    wl_out = rng.permutation(len(wl)).astype(np.int32)          # a node per list entry
    P = dict(B=B, F=F, beam=beam, rmax=rmax, ldt=ldt, n=n, segs=segs, msegs=msegs, ts=ts, keep=keep, tm_rows=tm_rows, n_nodes=len(wl),
             n_live_host=n_live, cnt_host=cnt, live_base_host=live_base)
    for name, a in dict(b2=b2, T=T, cnt=cnt, live_base=live_base, g0=g0, live=live, n_live=n_live, wl=np.asarray(wl, np.int32),
                        wl_out=wl_out, off=np.asarray(offs, np.int32), cidx=np.arange(ncell, dtype=np.int32),
                        sidx=np.tile(np.arange(B, dtype=np.int32), F), sent_len=np.asarray(LENS, np.int32)).items():
        P[name] = _dev(a)
    return P


def _p(P, name, elems=0):
    return P[name].data_ptr() + 4 * elems


@pytest.mark.parametrize("beam", [1, 3, 10, 16])
# the headline D-softmax* widths 200 / 100 / 50 AS LAUNCHED: the loader pads a segment's k to a multiple of 4 (50 -> 52, zero columns; the
# packers and the edge-logit launcher refuse any other k), so T rows are 352 floats and the blocks per row are 7 / 4 / 2: 26 groups
# k = 256: one segment that fills its last block (8 blocks, 16 groups).  232 / 232 / 40: 8 + 8 + 2 blocks = 36 groups, so a row takes TWO
# 32-group chunks of the packer (the fused kernel's chunk loop runs past its first turn) at ldt = 504, the widest rows 32 KB of LDS hold
@pytest.mark.parametrize("widths", [[200, 100, 52], [256], [232, 232, 40]], ids=["dsoftmax", "k256", "two-chunks"])
def test_fused_tail_leaves_the_bytes_of_the_two_launches(L, widths, beam):
    """(a) pack + edge logits against (b) the fused launch, frame by frame, whole buffers byte for byte.  The bases of the live cells are
    not multiples of 32 at any beam, and at beams 10 and 16 a cell straddles the first 32-row block of Tm (5 sentences x beam rows: at
    beams 1 and 3 a frame has fewer than 32 live rows)."""
    P = _problem(widths, beam)
    B, F, rmax, ldt, n = P["B"], P["F"], P["rmax"], P["ldt"], P["n"]
    ld_tm = L.jlm_mixed_t_stride(P["msegs"], n)
    assert ld_tm > 0
    if widths == [200, 100, 52]:
        assert ldt == 352
        assert [P["msegs"][i].ldb // 32 for i in range(n)] == [7, 4, 2]
    if widths == [232, 232, 40]:
        assert ldt == 504 and L.jlm_pack_edge_mx6_lds_bytes(ldt) == 32 * 1024
        assert sum(2 * (P["msegs"][i].ldb // 32) for i in range(n)) == 36
    lb, ch = P["live_base_host"], P["cnt_host"]
    if beam >= 10:          # some live cell straddles row 32 of the packed buffer
        assert any(lb[c] < 32 < lb[c] + ch[c] for c in range(F * B) if c // B < LENS[c % B] and ch[c]), (lb, ch)
    assert any(lb[c] % 32 for c in range(F * B) if c // B < LENS[c % B] and ch[c])
    tm_bytes, edge_bytes = P["tm_rows"] * ld_tm * 4, P["n_nodes"] * beam * 4
    for f in range(F):
        cell = f * B
        out = []
        for fused in (False, True):
            Tm = torch.full((tm_bytes,), SENTINEL, dtype=torch.uint8, device="cuda")
            edge = torch.full((edge_bytes,), SENTINEL, dtype=torch.uint8, device="cuda")
            if fused:
                rc = L.jlm_pack_edge_mx6(P["segs"], n, _p(P, "b2"), P["msegs"], P["ts"], n, _p(P, "T"), ldt, _p(P, "g0", cell), _p(P, "cnt"),
                                         _p(P, "cidx", cell), _p(P, "wl"), _p(P, "off"), _p(P, "sidx"), cell, _p(P, "wl_out"),
                                         edge.data_ptr(), beam, B, _p(P, "sent_len"), _p(P, "live_base", cell), f, Tm.data_ptr(), ld_tm, _st())
                assert rc == 0, rc
            else:
                rc = L.jlm_pack_t_mixed6(P["msegs"], P["ts"], n, _p(P, "T"), ldt, _p(P, "live", f * rmax), rmax, _p(P, "n_live", f),
                                         Tm.data_ptr(), ld_tm, _st())
                assert rc == 0, rc
                rc = L.jlm_edge_logits(P["segs"], n, _p(P, "b2"), _p(P, "T"), ldt, _p(P, "g0", cell), _p(P, "cnt"), _p(P, "cidx", cell),
                                       _p(P, "wl"), _p(P, "off"), _p(P, "sidx"), cell, _p(P, "wl_out"), edge.data_ptr(), beam, B, _st())
                assert rc == 0, rc
            torch.cuda.synchronize()
            out.append((Tm.cpu().numpy(), edge.cpu().numpy()))
        (tm_a, e_a), (tm_b, e_b) = out
        # (a) itself wrote what the frame needs: rows below n_live, and nothing in the spare block
        if P["n_live_host"][f]:
            assert (tm_a != SENTINEL).any()
        bad = np.flatnonzero(tm_a != tm_b)
        assert len(bad) == 0, ("packed rows differ", f, "first bytes", bad[:8].tolist(), "of", len(bad))
        bad = np.flatnonzero(e_a != e_b)
        assert len(bad) == 0, ("edge logits differ", f, "first bytes", bad[:8].tolist(), "of", len(bad))
        n_written = int((e_a.view(np.uint32) != 0xA5A5A5A5).sum())
        want = sum(N_WORDS[f][s] * int(ch[cell + s]) for s in range(B))
        assert n_written == want, (f, n_written, want)


def test_launcher_refuses_what_the_kernel_does_not_host(L):
    """beam > 16 and k > 256 are the two launches' business (-2), before anything is launched"""
    P = _problem([256], 3)
    n = P["n"]
    ld_tm = L.jlm_mixed_t_stride(P["msegs"], n)
    args = lambda beam: (P["segs"], n, _p(P, "b2"), P["msegs"], P["ts"], n, _p(P, "T"), P["ldt"], _p(P, "g0"), _p(P, "cnt"), _p(P, "cidx"),
                         _p(P, "wl"), _p(P, "off"), _p(P, "sidx"), 0, _p(P, "wl_out"), 0, beam, 0, _p(P, "sent_len"), _p(P, "live_base"), 0,
                         _p(P, "T"), ld_tm, _st())
    assert L.jlm_pack_edge_mx6(*args(16)) == 0           # (no groups: nothing is launched)
    assert L.jlm_pack_edge_mx6(*args(17)) == -2
    P["segs"][0].k = 260
    assert L.jlm_pack_edge_mx6(*args(16)) == -2
    P["segs"][0].k = 256


# ------------------------------------------------------------------------------------------------ decode level
_CHILD = r"""
import ctypes, json, sys
sys.path.insert(0, %(repo)r)
from tests.conftest import fixture_root
from tests import golden_cases as gc
from jlm_amd import _lib, config as jconfig
from jlm_amd.decoder import Decoder
out = {}
for name, fixture, kind, kwargs, spec in gc.DECODE_CASES:
    if name not in %(cases)r:
        continue
    f = fixture_root(fixture)
    jconfig.set_root(f["root"])
    dec = Decoder(1)
    sents = gc.case_sentences(spec, f["alphabet"])
    res = dec.decode_batch(sents, **kwargs)
    dev = dec.model.dev
    # does the fused launcher host this model at this beam?  (no groups: nothing is launched, the launcher only checks the shape --
    # the question jlm_decode_frames asks before it takes the fused launch)
    hosts = None
    if dev.mixed is not None and len(dev.mixed.segs) == len(dev.segments):
        n = len(dev.segments)
        seg = lambda d, B: _lib.Segment(int(d["v_start"]), int(d["v_end"]), int(d["k"]), int(d["t_off"]), B.data_ptr(), int(d["ldb"]))
        segs = (_lib.Segment * n)(*[seg(d, B) for d, B in zip(dev.segments, dev.seg_B)])
        msegs = (_lib.Segment * n)(*[seg(ms.seg, ms.packed) for ms in dev.mixed.segs])
        ts = (ctypes.c_float * n)(*[float(ms.t_scale) for ms in dev.mixed.segs])
        some = dev.b2.data_ptr()          # (any device address: with no groups nothing is read or written)
        hosts = _lib.lib().jlm_pack_edge_mx6(segs, n, dev.b2.data_ptr(), msegs, ts, n, some, dev.ldt, some, some, some, some, some, some, 0,
                                             some, some, int(kwargs.get("beam_width", 10)), 0, some, some, 0, some, dev.ld_tm, None)
    out[name] = dict(fmt=dev.mixed_fmt, mixed_idx=list(dev.mixed_idx or []), hosts=hosts, s8=[float(ms.s8) for ms in (dev.mixed.segs if dev.mixed else [])],
                     nbest=[[[float(s), list(w)] for s, w in r] for r in res])
print("RESULT " + json.dumps(out))
"""
DECODE_CASES = ["small-vtable/static", "mid-vtable/static"]


def _run_child(fuse):
    env = dict(os.environ)
    env.pop("JLM_FUSE_TAIL", None)
    if not fuse:
        env["JLM_FUSE_TAIL"] = "0"
    r = subprocess.run([sys.executable, "-c", _CHILD % dict(repo=REPO, cases=DECODE_CASES)], env=env, cwd=REPO, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


@pytest.fixture(scope="module")
def decoded():
    return _run_child(True), _run_child(False)


@pytest.mark.parametrize("case", DECODE_CASES)
def test_decode_is_identical_with_and_without_the_fused_tail(case, decoded, golden_decode):
    """n-best words and scores identical between the default (fused) decode and JLM_FUSE_TAIL=0, and within the suite's bar of the goldens"""
    from tests.test_gpu_decode import _check_nbest
    fused, two = decoded
    assert fused[case]["nbest"] == two[case]["nbest"]
    if case.startswith("mid-vtable"):                   # the headline model: every segment on mx6 rows, so the fused tail is what ran
        assert fused[case]["fmt"] == "mx6" and fused[case]["mixed_idx"] == [0, 1, 2], (fused[case]["fmt"], fused[case]["mixed_idx"])
        # ... and the launcher hosts the model's segments at the decode's beam (0; -2 would send the frame loop to the two launches and
        # make the comparison above one of a decode with itself), no segment on the int8 twin of its rows
        assert fused[case]["hosts"] == 0 and not any(fused[case]["s8"]), (fused[case]["hosts"], fused[case]["s8"])
    gold = golden_decode[case]
    for si, out in enumerate(fused[case]["nbest"]):
        n_kana = len(gold[si]["input"])
        _check_nbest([(s, w) for s, w in out], [(s, w) for s, w in gold[si]["nbest"]], (case, si), n_kana)
