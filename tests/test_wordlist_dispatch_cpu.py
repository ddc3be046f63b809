"""CPU-only: which kernel the word-list normaliser and the incremental back-fill launch (ABI 12: jlm_wordlist_lse_form,
jlm_wordlist_merge_form -- jlm_decode_frames, jlm_wordlist_lse(_perm) and the three launchers ask the same functions), for every segment
layout, split rows present or absent, weight-word lists on or off, beams around the 32-row blocks and the 64-row limit, list lengths
around the split kernels' bounds, and JLM_WORDLIST_MFMA unset, 0 and 1.  The library reads the variable once per process, hence one child
per setting.  Each child asks the real library and the numpy double (tests/fake_hip.py); the parent pins both against the table below."""
import json
import os
import subprocess
import sys

import pytest

from tests.fake_hip import WL_FORM, WL_FORMS, wordlist_lse_form, wordlist_merge_form

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# layout -> f32 segment widths (the split rows, where given, cover a single segment of the same k)
LAYOUTS = {"t4": [4], "t52": [52], "t100": [100], "t132": [132], "t192": [192], "t252": [252], "t256": [256], "t260": [260],
           "u512": [512], "dsoftmax": [200, 100, 52]}
BEAMS = [1, 32, 33, 64, 65, 1024]
MAX_WORDS = [0, 127, 128, 129, 4064, 4065]
SETTINGS = [None, "0", "1"]


def seg_rows(widths, V=3001):
    """(v_start, v_end, k, t_off, ldb) per f32 segment, and the split rows of a single segment (ldb = whole 16-value granules)"""
    out, t, n = [], 0, len(widths)
    cut = [V * i // n for i in range(n + 1)]
    for i, k in enumerate(widths):
        out.append((cut[i], cut[i + 1], k, t, k))
        t += k
    split = (0, V, widths[0], 0, (widths[0] + 15) // 16 * 16) if n == 1 else None
    return out, split, t + 4


_CHILD = r"""
import ctypes, json
from jlm_amd import _lib
from tests.fake_hip import FakeLib
from tests.test_wordlist_dispatch_cpu import BEAMS, LAYOUTS, MAX_WORDS, seg_rows
l = ctypes.CDLL(_lib.LIB_PATH)
for name in ("jlm_wordlist_lse_form", "jlm_wordlist_merge_form"):
    getattr(l, name).argtypes, getattr(l, name).restype = _lib._SIGS[name]
S = _lib.Segment
out = []
for lay, widths in sorted(LAYOUTS.items()):
    rows, split, ldt = seg_rows(widths)
    segs = (S * len(rows))(*[S(v0, v1, k, t, None, ldb) for v0, v1, k, t, ldb in rows])
    sp = (S * 1)(S(*split[:4], None, split[4])) if split else None
    for has_split in (0, 1):
        if has_split and sp is None:
            continue
        s = sp if has_split else None
        for perm in (0, 1):
            for beam in BEAMS:
                for mw in MAX_WORDS:
                    out.append([lay, has_split, perm, beam, mw,
                                l.jlm_wordlist_lse_form(segs, len(rows), s, perm, ldt, beam, mw),
                                FakeLib.jlm_wordlist_lse_form(segs, len(rows), s, perm, ldt, beam, mw),
                                l.jlm_wordlist_merge_form(segs, len(rows), s, ldt, beam, mw),
                                FakeLib.jlm_wordlist_merge_form(segs, len(rows), s, ldt, beam, mw)])
# refusals: no segment, k not a multiple of 4, ldt not a multiple of 4, f32 rows past LDS
bad = []
for widths, ldt in (([], 8), ([6], 8), ([8], 10), ([256], 2560 + 4)):
    segs = (S * max(len(widths), 1))(*[S(0, 100, k, 0, None, k + (k % 4 and 2)) for k in widths])
    bad.append([l.jlm_wordlist_lse_form(segs, len(widths), None, 1, ldt, 1024, 0),
                FakeLib.jlm_wordlist_lse_form(segs, len(widths), None, 1, ldt, 1024, 0)])
print(json.dumps({"forms": out, "bad": bad}))
"""


def pinned_lse(forced, lay, has_split, perm, beam, mw):
    """the kernel of every launch, spelled out (include/jlm_hip.h ids)"""
    widths = LAYOUTS[lay]
    if has_split and len(widths) == 1 and not perm and beam <= 64 and 128 <= mw <= 4064 and widths[0] <= 256:
        return WL_FORM["SPLIT"]
    if forced != "0" and not perm and len(widths) == 1 and beam <= 64 and widths[0] <= 256:
        return WL_FORM["MFMA"]
    return WL_FORM["F32"]


def pinned_merge(forced, lay, has_split, beam, mw):
    widths = LAYOUTS[lay]
    if has_split and len(widths) == 1 and beam <= 64 and mw <= 128 and widths[0] <= 256:
        return WL_FORM["MERGE_SPLIT"]
    return pinned_lse(forced, lay, has_split, 0, beam, mw)


@pytest.mark.parametrize("setting", SETTINGS, ids=lambda s: "unset" if s is None else "JLM_WORDLIST_MFMA=" + s)
def test_wordlist_forms(setting):
    env = {k: x for k, x in os.environ.items() if k != "JLM_WORDLIST_MFMA"}
    if setting is not None:
        env["JLM_WORDLIST_MFMA"] = setting
    r = subprocess.run([sys.executable, "-c", _CHILD], cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    n_single = sum(len(w) == 1 for w in LAYOUTS.values())
    assert len(got["forms"]) == (len(LAYOUTS) + n_single) * 2 * len(BEAMS) * len(MAX_WORDS)
    for lay, has_split, perm, beam, mw, form, fake, mform, mfake in got["forms"]:
        want = pinned_lse(setting, lay, has_split, perm, beam, mw)
        assert form == want == fake, (setting, lay, has_split, perm, beam, mw, form, fake, want)
        mwant = pinned_merge(setting, lay, has_split, beam, mw)
        assert mform == mwant == mfake, (setting, lay, has_split, beam, mw, mform, mfake, mwant)
    assert got["bad"] == [[-1, -1]] * 4


def test_every_form_is_reachable():
    """each of the four word-list kernels is what some launch of the table takes, and each default launch keeps the matrix pipe off
    only where JLM_WORDLIST_MFMA=0 says so"""
    seen = set()
    for forced in SETTINGS:
        for lay in LAYOUTS:
            for hs in (0, 1):
                for beam in BEAMS:
                    for mw in MAX_WORDS:
                        seen.add(pinned_lse(forced, lay, hs, 0, beam, mw))
                        seen.add(pinned_merge(forced, lay, hs, beam, mw))
    assert seen == set(range(len(WL_FORMS)))


def test_documented_boundaries():
    """the bounds include/jlm_hip.h states, on the numpy double (the library is pinned to it above)"""
    rows, split, ldt = seg_rows([132])
    assert wordlist_lse_form(rows, split, 0, ldt, 64, 128) == WL_FORM["SPLIT"]
    assert wordlist_lse_form(rows, split, 0, ldt, 64, 127) == WL_FORM["MFMA"]
    assert wordlist_lse_form(rows, split, 0, ldt, 64, 4064) == WL_FORM["SPLIT"]
    assert wordlist_lse_form(rows, split, 0, ldt, 64, 4065) == WL_FORM["MFMA"]
    assert wordlist_lse_form(rows, split, 0, ldt, 65, 200) == WL_FORM["F32"]
    assert wordlist_lse_form(rows, split, 1, ldt, 1, 200) == WL_FORM["F32"]          # weight-word lists: the f32 kernel only
    assert wordlist_lse_form(rows, split, 0, ldt, 1, 200, mfma=0) == WL_FORM["SPLIT"]   # the variable moves the f32 rows only
    assert wordlist_merge_form(rows, split, ldt, 64, 128) == WL_FORM["MERGE_SPLIT"]
    assert wordlist_merge_form(rows, split, ldt, 64, 129) == WL_FORM["SPLIT"]
    assert wordlist_merge_form(rows, None, ldt, 64, 5) == WL_FORM["MFMA"]
    # split rows of k > 256 (untied models): neither split kernel, the f32 kernel
    rows, split, ldt = seg_rows([512])
    assert wordlist_lse_form(rows, split, 0, ldt, 8, 300) == WL_FORM["F32"]
    assert wordlist_merge_form(rows, split, ldt, 8, 20) == WL_FORM["F32"]
