"""GPU: every H = 512 form of the decode's LSTM step (jlm_lstm_step_xg) launched the way the decode launches it.

The form a launch runs is the library's own answer (jlm_lstm_step_form, ABI 12): 1 gate_xg_u16_kernel, 3 gate_pu_kernel, 2 gate_ws_kernel,
4 gate_p2_kernel.  Each case asserts that answer against the restatement in tests/fake_hip.py, so a silent fall-through fails.  The axes:

* the f32 copy of h' -- none (tied, vtable and D-softmax models: the HF32 = false instantiations) and present (untied models);
* buffers stepped in place, or ping-pong (h_in != h_out, c_in != c_out; the outputs filled with a NaN sentinel beforehand);
* the launch's row bound x the device-side row count: 0, 1, one tile and one row more, every row-tile sequence one tile and one row
  more, a ragged count, bound - 1, bound, n_dev = NULL (jlm_lse_probe), and a count above the bound (the kernels clamp);
* saturated gates (|z| of 60-90 on a share of the gate columns, zero-state rows among them).

Every case checks h' and c' of the stepped rows against the f64 evaluation of the original f32 operands and against the numpy double
(FakeLib) on the same split rows, and every row that was not stepped bit for bit.  The split rows the epilogue writes are held to the
format: the split-pair invariants on every stepped row, and, where the f32 copy is written, bytes equal to split_pair(copy x h_scale).  One operand set per bound: a device count of n steps
the first n entries of the row list, so every case checks a prefix of one result.

Forced forms: test_gpu_kernels.py::test_lstm_step_xg_forced_forms runs this module (and test_lstm_step_xg) in a child per JLM_GATE_V
setting -- the variable is read once per process -- and test_lstm_step_xg_forms_agree compares what the children of forms 1-4 wrote
(the children run once per session, whichever test asks first)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
from jlm_amd import _lib                                                    # noqa: E402
from tests import operand_cases as OC                                       # noqa: E402
from tests.fake_hip import FakeLib, gate_v_env, lstm_step_form              # noqa: E402
from tests.test_gpu_kernels import _pack, _st, _unsplit, lstm_xg_f64        # noqa: E402

pytestmark = pytest.mark.gpu

H, S, HS = 512, 20, 2.0 ** 14
BOUNDS = (700, 2560, 5200, 10240, 20480)
FAKE_ALL = 5200                     # the numpy double on every row up to this bound, on a sample of rows above
OUT = os.environ.get("JLM_GATE_FORMS_OUT")          # set for the children of the forced-form tests
SAVE_BOUNDS = (2560, 5200, 20480)                   # the fixed inputs the forms are compared on
NAN_BITS = 0x7FC00000
RTOL, ATOL = 2e-5, 2e-6
FK = FakeLib()


def _geometry(form, bound):
    """(rows per tile, row-tile sequences per gate-column tile) of a launch: Q = min(row tiles, 16) for the 160-row tiles of forms 2 / 3,
    min(row tiles, 32) for the 128-row tiles of form 4 (form 1 has one tile per workgroup: the same counts as 2 / 3)"""
    bm, per = (128, 32) if form == 4 else (160, 16)
    return bm, min((bound + bm - 1) // bm, per)


def _counts(form, bound):
    bm, q = _geometry(form, bound)
    mid = (bound // 2) // bm * bm + bm // 2 + 7                              # ragged: inside a tile
    c = [0, 1, bm, bm + 1, q * bm, q * bm + 1, mid, bound - 1, bound]
    seen, out = set(), []
    for n in c:
        if 0 <= n <= bound and n not in seen:
            seen.add(n)
            out.append(n)
    return out + [None, bound + 37]                                          # n_dev = NULL; above the bound


def _cases(forced):
    """(bound, count, f32 copy, ping-pong, saturated, form) of every case under JLM_GATE_V = forced"""
    out = []
    for bound in BOUNDS:
        for hf32 in (False, True):
            form = lstm_step_form(H, 1, hf32, bound, forced)
            for n in _counts(form, bound):
                out.append((bound, n, hf32, False, False, form))
            for n in (_geometry(form, bound)[1] * _geometry(form, bound)[0] + 1, bound - 1, None):
                if n is None or n <= bound:
                    out.append((bound, n, hf32, True, False, form))
    for hf32 in (False, True):
        form = lstm_step_form(H, 1, hf32, 2560, forced)
        out += [(2560, 2559, hf32, pp, True, form) for pp in (False, True)]
    return out


def _case_id(c):
    bound, n, hf32, pp, sat, form = c
    return "f%d-B%d-n%s-%s-%s%s" % (form, bound, "NULL" if n is None else n, "f32" if hf32 else "nof32", "pingpong" if pp else "inplace",
                                    "-sat" if sat else "")


CASES = _cases(gate_v_env())


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return _lib.lib()


class _Set:
    """one operand set of a bound: state store of 2 x bound + 7 rows, the bound's rows at the top, their states below"""

    def __init__(self, L, bound, sat):
        rng = np.random.default_rng(bound + (99991 if sat else 0))
        V, G = 300, 2 * bound + 7
        self.bound, self.G = bound, G
        h_np = np.tanh(rng.standard_normal((G, H))).astype(np.float32)
        c_np = (rng.standard_normal((G, H)) * 0.5).astype(np.float32)
        W = (rng.standard_normal((4 * H, H)) * 0.08).astype(np.float32)
        xg = (rng.standard_normal((V, 4 * H)) * 0.6).astype(np.float32)
        if sat:
            # trained LSTMs run with |pre-activation| in the tens: a third of the words drive half of their gate columns to 60 .. 90
            hot = (np.arange(V) % 3 == 0)[:, None] & (rng.random((V, 4 * H)) < 0.5)
            xg = np.where(hot, np.sign(rng.standard_normal((V, 4 * H))) * rng.uniform(60, 90, (V, 4 * H)), xg).astype(np.float32)
        self.word = rng.integers(0, V, size=G).astype(np.int32)
        self.rows = (G - 1 - rng.permutation(bound)).astype(np.int32)
        prev = rng.integers(0, G - bound, size=G).astype(np.int32)
        prev[rng.random(G) < (0.25 if sat else 0.05)] = -1                   # zero-state rows, as the decode has them
        self.prev = prev
        self.hn, self.cn = lstm_xg_f64(h_np, c_np, W, xg, prev[self.rows], self.word[self.rows])
        self.hs0 = _pack(L, torch.as_tensor(h_np).cuda(), H, HS)
        self.c0 = torch.as_tensor(c_np).cuda()
        self.ws = _pack(L, torch.as_tensor(W).cuda(), H, 2.0 ** (S - 14))
        self.xg8 = torch.as_tensor(xg * np.float32(2.0 ** S)).cuda()
        self.rows_g, self.prev_g, self.word_g = (torch.as_tensor(x).cuda() for x in (self.rows, prev, self.word))
        torch.cuda.synchronize()
        # the numpy double on the same split rows: every position up to FAKE_ALL rows, a sample of 1 024 above
        pos = np.arange(bound) if bound <= FAKE_ALL else np.sort(rng.choice(bound, 1024, replace=False))
        hs_c, c_c, ws_c, xg_c = self.hs0.cpu(), torch.as_tensor(c_np), self.ws.cpu(), self.xg8.cpu()
        ho_c, co_c = torch.zeros_like(hs_c), torch.zeros_like(c_c)
        sub, prev_c, word_c = (torch.as_tensor(x) for x in (self.rows[pos], prev, self.word))
        assert FK.jlm_lstm_step_xg(hs_c.data_ptr(), c_c.data_ptr(), H, ho_c.data_ptr(), co_c.data_ptr(), sub.data_ptr(), prev_c.data_ptr(),
                                   word_c.data_ptr(), ws_c.data_ptr(), xg_c.data_ptr(), H, 2.0 ** -S, HS, None, len(pos), None, 0) == 0
        self.fake_pos = pos
        self.fake_h = _unsplit(ho_c[sub.long()]) / HS
        self.fake_c = co_c.numpy()[self.rows[pos]]


_SETS = {}


def _set(L, bound, sat):
    if (bound, sat) not in _SETS:
        _SETS.clear()                   # cases come bound by bound: one set resident at a time
        _SETS[(bound, sat)] = _Set(L, bound, sat)
    return _SETS[(bound, sat)]


def _bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("case", CASES, ids=[_case_id(c) for c in CASES])
def test_gate_form(L, case):
    bound, n, hf32, pingpong, sat, form = case
    d = _set(L, bound, sat)
    G = d.G
    assert L.jlm_lstm_step_form(H, 1, int(hf32), bound) == form
    h_in, c_in = d.hs0.clone(), d.c0.clone()
    if pingpong:
        h_out = torch.full_like(h_in, float("nan"))
        c_out = torch.full_like(c_in, float("nan"))
    else:
        h_out, c_out = h_in, c_in
    hf = torch.full((G, H), float("nan"), dtype=torch.float32, device="cuda") if hf32 else None
    nd = None if n is None else torch.tensor([n], dtype=torch.int32, device="cuda")
    assert L.jlm_lstm_step_xg(h_in.data_ptr(), c_in.data_ptr(), H, h_out.data_ptr(), c_out.data_ptr(), d.rows_g.data_ptr(),
                              d.prev_g.data_ptr(), d.word_g.data_ptr(), d.ws.data_ptr(), d.xg8.data_ptr(), H, 2.0 ** -S, HS,
                              hf.data_ptr() if hf32 else None, bound, None if nd is None else nd.data_ptr(), _st()) == 0
    torch.cuda.synchronize()
    m = bound if n is None else min(n, bound)
    sel = d.rows_g[:m].long()
    # stepped rows: the f64 evaluation of the original operands, and the numpy double on the same split rows
    h_got = _unsplit(h_out[sel]) / HS
    c_got = c_out[sel].cpu().numpy()
    np.testing.assert_allclose(h_got, d.hn[:m], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(c_got, d.cn[:m], rtol=RTOL, atol=ATOL)
    # the split-row epilogue writes the format (tests/operand_cases.py): every stepped row keeps the split rows' promises, and with the
    # f32 copy requested its bytes are split_pair(copy x h_scale) of that copy -- no tolerance
    h_bytes = h_out[sel].cpu().numpy().view(np.uint8).reshape(m, 4 * H)
    OC.check_split_pairs(h_bytes)
    if hf32:
        hf_got = hf[sel].cpu().numpy()
        np.testing.assert_allclose(hf_got, d.hn[:m], rtol=RTOL, atol=ATOL)
        OC.assert_bytes(h_bytes, OC.split_row_bytes(OC.f32_product(hf_got, HS)), "split h' against split_pair(f32 copy x h_scale) (row, byte)")
    k = d.fake_pos < m
    np.testing.assert_allclose(h_got[d.fake_pos[k]], d.fake_h[k], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(c_got[d.fake_pos[k]], d.fake_c[k], rtol=RTOL, atol=ATOL)
    if sat:
        assert np.isfinite(h_got).all() and np.isfinite(c_got).all()
        lim_c = np.isin(d.cn[:m].astype(np.float32), (-1.0, 0.0, 1.0))
        assert lim_c.sum() > 1000, lim_c.sum()                              # zero-state rows with both i and g saturated
        np.testing.assert_array_equal(c_got[lim_c], d.cn[:m].astype(np.float32)[lim_c])   # exact where the f64 result rounds to a limit
        lim_h = np.isin(d.hn[:m].astype(np.float32), (-1.0, 0.0, 1.0))
        np.testing.assert_array_equal(h_got[lim_h], d.hn[:m].astype(np.float32)[lim_h])
    # rows that were not stepped: bit for bit
    keep = torch.ones(G, dtype=torch.bool, device="cuda")
    keep[sel] = False
    if pingpong:
        assert torch.equal(_bits(h_in), _bits(d.hs0)) and torch.equal(_bits(c_in), _bits(d.c0)), "the inputs were written"
        assert (_bits(h_out)[keep] == NAN_BITS).all() and (_bits(c_out)[keep] == NAN_BITS).all(), "rows not stepped were written"
    else:
        assert torch.equal(_bits(h_out)[keep], _bits(d.hs0)[keep]), "split h of rows not stepped changed"
        assert torch.equal(_bits(c_out)[keep], _bits(d.c0)[keep]), "c of rows not stepped changed"
    if hf32:
        assert (_bits(hf)[keep] == NAN_BITS).all(), "f32 copy of rows not stepped was written"
    if OUT:
        with open(os.path.join(OUT, "cases.jsonl"), "a") as f:
            f.write(json.dumps({"id": _case_id(case), "form": form, "hf32": hf32}) + "\n")
        if bound in SAVE_BOUNDS and n == bound - 1 and not pingpong and not sat:
            np.savez(os.path.join(OUT, "B%d_%s.npz" % (bound, "f32" if hf32 else "nof32")), form=form,
                     h=_bits(h_out[sel]).cpu().numpy(), c=c_got)


# ---------------------------------------------------------------------------------------------------- forced forms, in child processes

_CHILDREN = {"1": {"JLM_GATE_V": "1"}, "2": {"JLM_GATE_V": "2"}, "3": {"JLM_GATE_V": "3"}, "4": {"JLM_GATE_V": "4"},
             "2-ws_l7": {"JLM_GATE_V": "2", "JLM_GATE_WS_L": "7"}, "2-ws_cx2": {"JLM_GATE_V": "2", "JLM_GATE_WS_CX": "2"},
             "2-ws_cx8": {"JLM_GATE_V": "2", "JLM_GATE_WS_CX": "8"}, "2-ws_cx16": {"JLM_GATE_V": "2", "JLM_GATE_WS_CX": "16"}}
_RUNS = {}


def _child(label, tmp_path_factory):
    """run this module and test_lstm_step_xg under one forced setting (once per session; one child at a time).  After a child that
    died of a signal or ran out of time, no further child starts."""
    if label not in _RUNS:
        bad = [k for k, r in _RUNS.items() if r["fatal"]]
        if bad:
            pytest.fail("not started: child %s ended abnormally" % bad[0])
        out = str(tmp_path_factory.mktemp("gate_v" + label))
        env = {k: v for k, v in os.environ.items() if not k.startswith("JLM_GATE")}
        env.update(_CHILDREN[label], JLM_GATE_FORMS_OUT=out)
        here = os.path.dirname(os.path.abspath(__file__))
        try:
            r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), os.path.join(here, "test_gpu_kernels.py"), "-q",
                                "-x", "-m", "gpu", "-k", "test_gate_form or (test_lstm_step_xg and not forced and not agree)"],
                               env=env, capture_output=True, text=True, timeout=900)
            rec = {"rc": r.returncode, "log": r.stdout[-3000:] + r.stderr[-2000:], "summary": r.stdout[-1000:], "fatal": r.returncode < 0}
        except subprocess.TimeoutExpired as e:
            rec = {"rc": None, "log": "timed out: %r" % (e.stdout[-2000:] if e.stdout else ""), "summary": "", "fatal": True}
        rec["out"] = out
        path = os.path.join(out, "cases.jsonl")
        rec["cases"] = [json.loads(x) for x in open(path)] if os.path.exists(path) else []
        _RUNS[label] = rec
    return _RUNS[label]


def check_forced_child(label, tmp_path_factory):
    """test_gpu_kernels.py::test_lstm_step_xg_forced_forms: the child of one forced setting passed, ran at least every case its form
    serves -- all of them for 1 .. 3, those without the f32 copy for 4 -- and each of them launched the forced form"""
    r = _child(label, tmp_path_factory)
    assert r["rc"] == 0, r["log"]
    assert " passed" in r["summary"] and "failed" not in r["summary"], r["summary"]
    forced = int(_CHILDREN[label]["JLM_GATE_V"])
    eligible = [c for c in _cases(forced) if forced != 4 or not c[2]]
    ran = {c["id"]: c for c in r["cases"]}
    served = [c for c in ran.values() if forced != 4 or not c["hf32"]]
    assert len(served) >= len(eligible), (len(served), len(eligible))
    assert all(c["form"] == forced for c in served), [c["id"] for c in served if c["form"] != forced]
    assert all(_case_id(c) in ran for c in eligible)


def test_lstm_step_xg_forms_agree(tmp_path_factory):
    """h' and c' of forms 1 .. 4 on the fixed inputs of the 2 560-, 5 200- and 20 480-row cases (device count bound - 1, in place), with
    and without the f32 copy.  Measured on the MI355X: bit for bit, every bound and both copy settings, so identity is what is pinned (a
    schedule change that reorders a form's accumulation shows up here first).  Whether the copy is written must not change h' or c' in
    any form: both are instantiations of one schedule."""
    if os.environ.get("JLM_GATE_FORMS_OUT"):
        pytest.skip("inside a child")
    runs = {v: _child(v, tmp_path_factory) for v in ("1", "2", "3", "4")}
    for v, r in runs.items():
        assert r["rc"] == 0, (v, r["log"])
    for bound in SAVE_BOUNDS:
        ref = np.load(os.path.join(runs["1"]["out"], "B%d_nof32.npz" % bound))
        assert int(ref["form"]) == 1
        for v, r in runs.items():
            for copy in ("nof32", "f32"):
                got = np.load(os.path.join(r["out"], "B%d_%s.npz" % (bound, copy)))
                form = int(got["form"])
                assert form == (int(v) if copy == "nof32" or v != "4" else lstm_step_form(H, 1, 1, bound, -1))
                assert got["h"].shape == ref["h"].shape
                ulp_h = _ulps(got["h"].view(np.int16), ref["h"].view(np.int16))
                ulp_c = _ulps(got["c"].view(np.int32), ref["c"].view(np.int32))
                assert ulp_h == 0 and ulp_c == 0, (bound, v, copy, form, "largest difference in ulps: h' %d, c' %d" % (ulp_h, ulp_c))
            a, b = (np.load(os.path.join(r["out"], "B%d_%s.npz" % (bound, x))) for x in ("nof32", "f32"))
            if int(a["form"]) == int(b["form"]):
                np.testing.assert_array_equal(a["h"], b["h"])
                np.testing.assert_array_equal(a["c"], b["c"])


def _ulps(a, b):
    """largest distance in units in the last place between two arrays of raw bits: int32 words of f32 values, or int16 words of f16
    values (the halves of split rows, each compared as f16)"""
    if a.size == 0:
        return 0
    sign = 0x7FFF if a.dtype == np.int16 else 0x7FFFFFFF
    a, b = a.astype(np.int64), b.astype(np.int64)
    ka = np.where(a < 0, -(a & sign), a)
    kb = np.where(b < 0, -(b & sign), b)
    return int(np.abs(ka - kb).max())
