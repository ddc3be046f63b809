"""GPU: the logit GEMMs of a row set exactly as rows_logits (csrc/jlm_decode.hip) launches them for generate and complete: one
jlm_gemm_nt per vocabulary segment with A = T + t_off (row stride ldt), B = the segment's block, C = logits + v_start (row stride
ld_logits = V rounded up to 4), bias = b2 + v_start, N = v_end - v_start, K = the segment's k, no row maps, no device count.

The vocabularies are odd (2 003, 2 011) and the cuts are no multiples of 4 (v_start % 4 = 1, 2, 3; one segment of 8 x 64 + 1 words: its
last tile is a single column), so every segment's C and bias start at an unaligned column, neighbouring segments write next to each
other inside one row, and ld_logits > V leaves padding columns.  The buffer is filled with one NaN bit pattern and has guard rows:
after each single launch exactly that segment's cells [0:n_rows, v_start:v_end] have changed, after all of them every cell of
[0:n_rows, 0:V] is within test_gpu_kernels.py::test_gemm_nt's bar (2e-5 x max(1, max |want|)) of the float64 restatement
(FakeLib.jlm_gemm_nt, run the same way) and every other cell still holds the pattern.  A store one column too far or a bias read at the
wrong offset lands in a neighbour's columns or in the padding.

test_tile_form_switch runs both sides of jlm_gemm_nt's 64 x 64 / 128 x 128 tile switch (fewer than 512 tiles of 128 x 128) at these
operands: M = 897 with N = 8 064 (504 tiles) and N = 8 065 (512)."""
import zlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")
from jlm_amd import _lib                              # noqa: E402
from tests.fake_hip import FakeLib                    # noqa: E402
from tests.test_gpu_kernels import _st                # noqa: E402

pytestmark = pytest.mark.gpu

FK = FakeLib()
NAN_BITS = np.uint32(0x7FC00000)
GUARD_ROWS = 3
LAYOUTS = {"s32_16_8": [32, 16, 8], "dsoftmax": [200, 100, 52], "k36": [36], "k4": [4], "k512": [512]}
# three-segment cuts per vocabulary: 501 / 1 203 (v_start % 4 = 1, 3); 513 / 1 218 (v_start % 4 = 1, 2; the first segment has 8 x 64 + 1 words)
CUTS = {2003: (501, 1203), 2011: (513, 1218)}
ROWS = (1, 63, 64, 65, 130)


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return _lib.lib()


class Model:
    """the output side of a model as rows_logits sees it: segments over [0, V) with the given cuts, T rows, b2 -- host and device"""

    def __init__(self, widths, cuts, n_rows, seed=0):
        rng = np.random.default_rng(zlib.crc32(repr((widths, cuts, n_rows, seed)).encode()))
        self.cuts, self.V, self.n_rows = list(cuts), cuts[-1], n_rows
        self.ldt = sum(widths) + 4
        self.ld = (self.V + 3) // 4 * 4
        self.T = rng.standard_normal((n_rows + GUARD_ROWS, self.ldt)).astype(np.float32)
        self.b2 = rng.standard_normal(self.V).astype(np.float32)
        self.keep, self.segs = [], {False: [], True: []}
        off = 0
        for i, k in enumerate(widths):
            blk = (rng.standard_normal((cuts[i + 1] - cuts[i], k)) * 0.3).astype(np.float32)
            for cuda in (False, True):
                t = torch.as_tensor(blk).cuda() if cuda else torch.as_tensor(blk)
                self.keep.append(t)
                self.segs[cuda].append(_lib.Segment(cuts[i], cuts[i + 1], k, off, t.data_ptr(), k))
            off += k
        self.dev = {False: (torch.as_tensor(self.T), torch.as_tensor(self.b2)),
                    True: (torch.as_tensor(self.T).cuda(), torch.as_tensor(self.b2).cuda())}

    def buffer(self, cuda):
        t = torch.empty((self.n_rows + GUARD_ROWS, self.ld), dtype=torch.float32)
        t.view(torch.int32).fill_(int(NAN_BITS))
        return t.cuda() if cuda else t

    def launch(self, lib, cuda, i, logits):
        """segment i's launch of rows_logits"""
        sg = self.segs[cuda][i]
        T, b2 = self.dev[cuda]
        return lib.jlm_gemm_nt(T.data_ptr() + 4 * sg.t_off, self.ldt, None, sg.B, sg.ldb, None, logits.data_ptr() + 4 * sg.v_start, self.ld,
                               None, b2.data_ptr() + 4 * sg.v_start, self.n_rows, sg.v_end - sg.v_start, sg.k, None, _st() if cuda else 0)


def _check_segments(L, M, order):
    """the launches of `order` one after the other; after each, exactly its cells have changed and they are right"""
    want_t, got_t = M.buffer(False), M.buffer(True)
    written = np.zeros((M.n_rows + GUARD_ROWS, M.ld), dtype=bool)
    before = got_t.cpu().numpy().view(np.uint32).copy()
    worst = 0.0
    for i in order:
        assert M.launch(FK, False, i, want_t) == 0
        assert M.launch(L, True, i, got_t) == 0
        torch.cuda.synchronize()
        sg = M.segs[False][i]
        got, want = got_t.cpu().numpy(), want_t.numpy()
        bits = got.view(np.uint32)
        mine = np.zeros_like(written)
        mine[:M.n_rows, sg.v_start:sg.v_end] = True
        changed = np.argwhere((bits != before) & ~mine)
        assert len(changed) == 0, ("segment", i, "cells changed outside its columns (row, column):", changed[:8].tolist(), len(changed))
        g, w = got[:M.n_rows, sg.v_start:sg.v_end], want[:M.n_rows, sg.v_start:sg.v_end]
        assert np.isfinite(g).all(), ("segment", i, np.argwhere(~np.isfinite(g))[:8].tolist())
        err = float(np.abs(g - w).max())
        assert err <= 2e-5 * max(1.0, float(np.abs(w).max())), ("segment", i, err)
        worst = max(worst, err)
        written |= mine
        before = bits.copy()
    got, want = got_t.cpu().numpy(), want_t.numpy()
    assert (got.view(np.uint32)[~written] == NAN_BITS).all()
    assert (want.view(np.uint32)[~written] == NAN_BITS).all()
    if len(order) == len(M.segs[False]):
        assert written[:M.n_rows, :M.V].all() and not written[M.n_rows:].any() and not written[:, M.V:].any()
        assert np.isfinite(got[:M.n_rows, :M.V]).all()
        assert np.abs(got[:M.n_rows, :M.V] - want[:M.n_rows, :M.V]).max() <= 2e-5 * max(1.0, float(np.abs(want[:M.n_rows, :M.V]).max()))
    return worst


@pytest.mark.parametrize("n_rows", ROWS)
@pytest.mark.parametrize("V", sorted(CUTS))
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_row_logits(L, layout, V, n_rows):
    widths = LAYOUTS[layout]
    cuts = (0,) + CUTS[V] + (V,) if len(widths) == 3 else (0, V)
    assert len(widths) == 1 or {c % 4 for c in cuts[1:-1]} <= {1, 2, 3}
    assert V % 4 == 3 and (V + 3) // 4 * 4 > V
    M = Model(widths, cuts, n_rows)
    _check_segments(L, M, list(range(len(widths))))
    if len(widths) > 1:
        # the last segment first: a segment's launch alone, with NaN on both sides of its columns
        _check_segments(L, M, list(range(len(widths)))[::-1])


def test_a_segment_whose_last_tile_is_one_column(L):
    assert (CUTS[2011][0] - 0) % 64 == 1
    for n_rows in (1, 65):
        M = Model([200, 100, 52], (0,) + CUTS[2011] + (2011,), n_rows)
        _check_segments(L, M, [0])
        _check_segments(L, M, [1])


def _tiles128(M, N):
    return ((M + 127) // 128) * ((N + 127) // 128)


@pytest.mark.parametrize("N", [8064, 8065])
def test_tile_form_switch(L, N):
    """M = 897 rows (a last row tile of one row), K = 52, a segment starting at column 5 with its bias: 504 tiles of 128 x 128 run the
    64 x 64 form, 512 the 128 x 128 form (jlm_gemm_nt: tiles128 < 512)"""
    rows = 897
    assert _tiles128(rows, 8064) == 504 < 512 == _tiles128(rows, 8065)
    M = Model([4, 52], (0, 5, 5 + N), rows)
    assert M.ld > M.V or M.V % 4 == 0
    _check_segments(L, M, [1])
    _check_segments(L, M, [1, 0])
