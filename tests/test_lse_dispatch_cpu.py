"""CPU-only: which kernel the vocabulary normaliser and the T projection launch (ABI 12: jlm_vocab_lse_mixed_form,
jlm_vocab_lse_split_form, jlm_gemm_nt_split_form -- the launchers ask the same functions), with every documented A/B setting unset and
forced.  The library reads JLM_MX_WIDE, JLM_MX6_WIDE, JLM_LSE_WAVES, JLM_T_STAGES and JLM_T_XCD once per process, hence one child per
setting.  Each child asks the real library and the numpy double (tests/fake_hip.py); the parent pins both against the table below.
Documented fall-throughs: JLM_MX_WIDE=1 on a shape the wide kernel does not host stays on the eight-wave kernel; the wide int8
D-softmax* launch has no fixed-reference form and ignores the flag; mx6 rows at k = 512 are refused."""
import json
import os
import subprocess
import sys

import pytest

from tests.fake_hip import MX_FORM, MX_FORMS, T_FORMS, gemm_nt_split_form, lse_mixed_form, lse_split_form

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _seg_rows(widths, V=3001):
    """(v_start, v_end, k, t_off, ldb) per segment as the packer lays the mixed rows out: bias columns where k + 2 fits the blocks of k,
    none for a contraction that fills its last block (k a multiple of 32)"""
    out, t, n = [], 0, len(widths)
    cut = [V * i // n for i in range(n + 1)]
    for i, k in enumerate(widths):
        nb = k // 32 if k % 32 == 0 else (k + 2 + 31) // 32
        out.append((cut[i], cut[i + 1], k, t, 32 * nb))
        t += k
    return out


# layout -> the shape class it hosts
LAYOUTS = {"dsoftmax": [200, 100, 52], "g252": [252], "g4_36": [4, 36], "tied": [256], "xb128_64": [128, 64], "k512": [512]}
SETTINGS = [None, ("JLM_MX_WIDE", "-1"), ("JLM_MX_WIDE", "0"), ("JLM_MX_WIDE", "1"), ("JLM_MX6_WIDE", "-1"), ("JLM_MX6_WIDE", "0"),
            ("JLM_MX6_WIDE", "1"), ("JLM_LSE_WAVES", "4"), ("JLM_T_STAGES", "4"), ("JLM_T_XCD", "0")]
T_SHAPES = [(1, 8), (700, 352), (2560, 256), (2560, 352), (4096, 256), (5200, 256), (10240, 256), (20480, 256), (20480, 352),
            (4096, 2048), (20480, 512)]

_CHILD = r"""
import ctypes, json
from jlm_amd import _lib
from tests.fake_hip import FakeLib
from tests.test_lse_dispatch_cpu import LAYOUTS, T_SHAPES, _seg_rows
l = ctypes.CDLL(_lib.LIB_PATH)
for name in ("jlm_vocab_lse_mixed_form", "jlm_vocab_lse_split_form", "jlm_gemm_nt_split_form"):
    getattr(l, name).argtypes, getattr(l, name).restype = _lib._SIGS[name]
F = ctypes.c_float
mixed = []
for lay, widths in sorted(LAYOUTS.items()):
    rows = _seg_rows(widths)
    n = len(rows)
    segs = (_lib.Segment * n)(*[_lib.Segment(v0, v1, k, t, None, ldb) for v0, v1, k, t, ldb in rows])
    for fmt in ("int8", "mx6"):
        for d in (1.0, 2.0 ** -14):
            for fr in (0, 1):
                for hb in (0, 1):
                    s8 = (F * n)(*([0.0] * n if fmt == "mx6" else [2.0 ** -5] * n))
                    ds = (F * n)(*([d] * n))
                    mixed.append([lay, fmt, d, fr, hb, l.jlm_vocab_lse_mixed_form(segs, ds, s8, hb, n, fr),
                                  FakeLib.jlm_vocab_lse_mixed_form(segs, ds, s8, hb, n, fr)])
# refusals: no segment, formats mixed within a launch
segs = (_lib.Segment * 3)(*[_lib.Segment(v0, v1, k, t, None, ldb) for v0, v1, k, t, ldb in _seg_rows(LAYOUTS["dsoftmax"])])
odd = [[l.jlm_vocab_lse_mixed_form(segs, (F * 3)(1, 1, 1), (F * 3)(*s8), 0, n, 0),
        FakeLib.jlm_vocab_lse_mixed_form(segs, (F * 3)(1, 1, 1), (F * 3)(*s8), 0, n, 0)] for s8, n in (([0.03] * 3, 0), ([0.0, 0.03, 0.03], 3))]
gemm = [[M, N, l.jlm_gemm_nt_split_form(M, N), FakeLib.jlm_gemm_nt_split_form(M, N)] for M, N in T_SHAPES]
print(json.dumps({"mixed": mixed, "odd": odd, "split": [l.jlm_vocab_lse_split_form(), FakeLib.jlm_vocab_lse_split_form()], "gemm": gemm}))
"""


def _mx(name):
    return MX_FORM[name]


def _pinned_mixed(env, lay, fmt, d, fr, hb):
    """the kernel of every launch, spelled out per setting (include/jlm_hip.h ids)"""
    mxw = int(env.get("JLM_MX_WIDE", "-1"))
    mx6w = int(env.get("JLM_MX6_WIDE", "-1"))
    xb = lay in ("tied", "xb128_64", "k512")
    if xb and not hb:
        return -2                                                   # external biases need bias2
    if fmt == "mx6":
        fr6 = fr and d == 1.0
        if lay == "k512":
            return -2                                               # mx6 rows hold at most eight blocks
        if lay == "dsoftmax":
            if mx6w == 1:
                return _mx("MX6W_KERNEL_DSOFTMAX_FR" if fr6 else "MX6W_KERNEL_DSOFTMAX")
            return _mx("MX6_KERNEL_DSOFTMAX_FR" if fr6 else "MX6_KERNEL_DSOFTMAX")
        if lay == "tied":
            if mx6w == 0:
                return _mx("MX6_KERNEL_TIED_FR" if fr6 else "MX6_KERNEL_TIED")
            return _mx("MX6W_KERNEL_TIED_FR" if fr6 else "MX6W_KERNEL_TIED")
        return _mx("MX6_KERNEL_GENERIC_XB" if lay == "xb128_64" else "MX6_KERNEL_GENERIC")
    if lay == "dsoftmax":
        return _mx("MXW_KERNEL_DSOFTMAX" if mxw == 1 else "MX_KERNEL_DSOFTMAX")      # (the wide D-softmax* launch ignores fixed_ref)
    if lay == "tied":
        if mxw == 0:
            return _mx("MX_KERNEL_TIED")
        return _mx("MXW_KERNEL_TIED_FR" if fr else "MXW_KERNEL_TIED")
    if lay == "k512":
        return _mx("MXW_KERNEL_K512_FR" if fr else "MXW_KERNEL_K512")
    return _mx("MX_KERNEL_GENERIC_XB" if lay == "xb128_64" else "MX_KERNEL_GENERIC")  # (JLM_MX_WIDE=1 does not move these)


def _pinned_gemm(env, M, N):
    stages, xcd = int(env.get("JLM_T_STAGES", "3")), int(env.get("JLM_T_XCD", "1"))
    tiles64 = ((M + 63) // 64) * ((N + 63) // 64)
    if tiles64 <= 256 and stages == 3:
        return T_FORMS.index("SPLIT3_LINEAR" if xcd == 0 else "SPLIT3_XCD")
    return T_FORMS.index("CFG64" if ((M + 127) // 128) * ((N + 127) // 128) < 512 else "CFG128")


@pytest.mark.parametrize("setting", SETTINGS, ids=lambda s: "unset" if s is None else "%s=%s" % s)
def test_lse_forms(setting):
    env = {k: x for k, x in os.environ.items() if k not in ("JLM_MX_WIDE", "JLM_MX6_WIDE", "JLM_LSE_WAVES", "JLM_T_STAGES", "JLM_T_XCD")}
    forced = {} if setting is None else {setting[0]: setting[1]}
    env.update(forced)
    r = subprocess.run([sys.executable, "-c", _CHILD], cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert len(got["mixed"]) == len(LAYOUTS) * 2 * 2 * 2 * 2
    for lay, fmt, d, fr, hb, form, fake in got["mixed"]:
        want = _pinned_mixed(forced, lay, fmt, d, fr, hb)
        assert form == want, (forced, lay, fmt, d, fr, hb, form, want)
        assert fake == want, (forced, lay, fmt, d, fr, hb, fake, want)                # the numpy double agrees
        assert want < 0 or 0 <= want < len(MX_FORMS)
    assert got["odd"] == [[-1, -1], [-2, -2]]
    waves = 4 if forced.get("JLM_LSE_WAVES") == "4" else 8
    assert got["split"] == [waves, waves]
    assert lse_split_form(int(forced.get("JLM_LSE_WAVES", "8"))) == waves
    for M, N, form, fake in got["gemm"]:
        want = _pinned_gemm(forced, M, N)
        assert form == want == fake, (forced, M, N, form, fake, want)


def test_every_form_is_reachable():
    """each of the 19 mixed / mx6 kernels and the four T-projection paths is what some setting launches"""
    seen = set()
    for setting in SETTINGS:
        forced = {} if setting is None else {setting[0]: setting[1]}
        for lay in LAYOUTS:
            for fmt in ("int8", "mx6"):
                for d in (1.0, 2.0 ** -14):
                    for fr in (0, 1):
                        seen.add(_pinned_mixed(forced, lay, fmt, d, fr, 1))
    assert seen - {-2} == set(range(len(MX_FORMS)))
    t = {_pinned_gemm({} if s is None else {s[0]: s[1]}, M, N) for s in SETTINGS for M, N in T_SHAPES}
    assert t == set(range(len(T_FORMS)))


def test_documented_fall_throughs():
    """INTEGRATION.md, JLM_MX_WIDE / JLM_MX6_WIDE / JLM_MX_FIXREF, on the numpy double (the library is pinned to it above)"""
    ds = _seg_rows([200, 100, 52])
    g = _seg_rows([252])
    # JLM_MX_WIDE=1 on a shape the wide kernel does not host: the eight-wave kernel
    assert lse_mixed_form(g, [1.0], [0.03], 0, 0, mx_wide=1) == _mx("MX_KERNEL_GENERIC")
    # the wide int8 D-softmax* launch ignores fixed_ref
    assert lse_mixed_form(ds, [1.0] * 3, [0.03] * 3, 0, 1, mx_wide=1) == _mx("MXW_KERNEL_DSOFTMAX")
    # the eight-wave int8 D-softmax* launch has no fixed-reference form either
    assert lse_mixed_form(ds, [1.0] * 3, [0.03] * 3, 0, 1) == _mx("MX_KERNEL_DSOFTMAX")
    # mx6 rows at k = 512 are refused
    assert lse_mixed_form(_seg_rows([512]), [1.0], [0.0], 1, 0) == -2
    # mx6 fixed-reference forms only where every descale is 1
    assert lse_mixed_form(ds, [1.0, 1.0, 0.5], [0.0] * 3, 0, 1) == _mx("MX6_KERNEL_DSOFTMAX")
