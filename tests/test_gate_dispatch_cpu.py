"""CPU-only: which kernel form jlm_lstm_step_xg launches (jlm_lstm_step_form, ABI 12), with JLM_GATE_V unset and forced to each
H = 512 form.  The library reads the variable once per process, hence one child per setting.  A forced form that cannot serve a
launch -- 2 / 3 without a row list, 4 without a row list or with the f32 copy of h' -- takes the row-bound default."""
import json
import os
import subprocess
import sys

import pytest

from tests.fake_hip import lstm_step_form

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS = (1, 4095, 4096, 16383, 16384, 20480)

_CHILD = r"""
import ctypes, json
from jlm_amd import _lib
from tests.fake_hip import FakeLib
l = ctypes.CDLL(_lib.LIB_PATH)
f = l.jlm_lstm_step_form
f.argtypes = [ctypes.c_int] * 4
f.restype = ctypes.c_int
out = []
for H in (64, 512, 500, 0):
    for r in (0, 1):
        for h in (0, 1):
            for b in %r:
                out.append([H, r, h, b, f(H, r, h, b), FakeLib.jlm_lstm_step_form(H, r, h, b)])
print(json.dumps(out))
""" % (BOUNDS,)


def _default(rows, hf32, bound):
    if not rows:
        return 1
    return 1 if bound < 4096 else 3 if bound < 16384 else 2


# the form of every H = 512 launch, spelled out per setting: (rows, f32 copy, bound) -> form
def _pinned(v, rows, hf32, bound):
    if v == "1":
        return 1
    if v in ("2", "3"):
        return int(v) if rows else 1
    if v == "4":
        return 4 if rows and not hf32 else _default(rows, hf32, bound)
    return _default(rows, hf32, bound)


@pytest.mark.parametrize("v", [None, "0", "1", "2", "3", "4", "9"])
def test_lstm_step_form(v):
    env = {k: x for k, x in os.environ.items() if k != "JLM_GATE_V"}
    if v is not None:
        env["JLM_GATE_V"] = v
    r = subprocess.run([sys.executable, "-c", _CHILD], cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert len(got) == 4 * 2 * 2 * len(BOUNDS)
    forced = -1 if v is None else int(v)
    for H, rows, hf32, bound, form, fake in got:
        want = -1 if H in (0, 500) else 0 if H == 64 else _pinned(v, rows, hf32, bound)
        assert form == want, (v, H, rows, hf32, bound, form, want)
        assert fake == want, (v, H, rows, hf32, bound, fake, want)                 # the numpy double agrees
        assert lstm_step_form(H, rows, hf32, bound, forced) == want


def test_documented_fall_through():
    """INTEGRATION.md, JLM_GATE_V: launches with the f32 copy under JLM_GATE_V=4 take the default at every bound (2 at 20 480 rows),
    not the one-tile kernel"""
    assert lstm_step_form(512, 1, 1, 20480, 4) == 2
    assert lstm_step_form(512, 1, 1, 10240, 4) == 3
    assert lstm_step_form(512, 1, 0, 20480, 4) == 4
    assert lstm_step_form(512, 0, 0, 20480, 2) == 1
