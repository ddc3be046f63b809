"""CPU: every packer of tests/fake_hip.py -- the numpy restatement the CPU suite runs the host path on, and the GPU suite compares the
kernels with -- against the exact definitions of the operand formats in tests/operand_cases.py, byte for byte, on the cases
tests/test_gpu_operand_formats.py runs on the device.  A restatement that agrees with the definitions here and a device packer that agrees
with them there write the same bytes."""
import numpy as np
import pytest

from tests import operand_cases as C
from tests.fake_hip import FakeLib

FK = FakeLib()
MEM = C.HostMem


def test_split_pair_and_its_invariants():
    rng = np.random.default_rng(1)
    x = C.split_values(rng, 40, 64, 1.0)
    hi, lo = C.split_pair(x)
    assert (hi == x.astype(np.float16)).all()
    assert np.abs(x.astype(np.float64) - hi.astype(np.float64) - lo.astype(np.float64)).max() <= 2.0 ** -22 * np.abs(x).max()
    bits = C.split_row_bytes(x)
    C.check_split_pairs(bits)
    # a row whose lo was taken against ANOTHER hi (the 2^-11 error of csrc/jlm_common.h jlm_split2's comment) breaks them
    bad = C.split_row_bytes(np.full((1, 8), 1025.25, np.float32)).copy()
    v = bad.view(np.float16)
    assert v[0, 0] == 1025 and v[0, 8] == 0.25
    C.check_split_pairs(bad)
    v[0, 8] = 0.75                                 # hi + lo rounds to 1026: lo belongs to another hi
    with pytest.raises(AssertionError):
        C.check_split_pairs(bad)
    v[0, 8] = np.inf
    with pytest.raises(AssertionError):
        C.check_split_pairs(bad)
    # the one exception: a correct lo that was rounded up to exactly half an ulp of an odd hi
    x = np.full((1, 8), np.float32(float.fromhex("0x1.ac5ffep-3")))
    ok = C.split_row_bytes(x)
    assert ok.view(np.float16)[0, 8] == 2.0 ** -14
    C.check_split_pairs(ok)


def test_split_invariant_on_every_f16_hi():
    """check_split_pairs' one comparison on the bit fields against the sum formed and rounded (it asserts that they agree), for every
    finite hi with lo at 0, 1/8, 1/4, 0.49, 1/2, just above 1/2, 3/4 and 1 of hi's ulp, both signs; what must pass passes"""
    hb = np.arange(0x10000, dtype=np.uint16)
    hb = hb[(hb & 0x7c00) != 0x7c00]
    h = hb.view(np.float16)
    n = len(h) // 8 * 8
    with np.errstate(over="ignore"):
        sp = np.spacing(np.abs(h)).astype(np.float64)
    sp = np.where(np.isfinite(sp), sp, 32.0)
    passed = set()
    for f in (0.0, 0.125, 0.25, 0.49, 0.5, 0.5000001, 0.75, 1.0, -0.125, -0.25, -0.49, -0.5, -0.75, -1.0):
        rows = np.zeros((n // 8, 2, 8), np.float16)
        rows[:, 0, :] = h[:n].reshape(-1, 8)
        rows[:, 1, :] = (f * sp).astype(np.float16)[:n].reshape(-1, 8)
        try:
            C.check_split_pairs(rows.view(np.uint8).reshape(1, -1))
            passed.add(f)
        except AssertionError as e:
            assert "lo moves hi" in str(e), str(e)[:200]
    assert passed == {0.0, 0.125, 0.25, -0.125, -0.25}         # (0.49 and 0.5 of the ulp are too far on the inner side of a power of two)


def test_int8_planes_ties_and_clip():
    hi = np.array([0.5, 1.5, 2.5, -0.5, -1.5, 126.5, 127.5, 4000.0, -4000.0], np.float16)
    lo = np.array([0.5, 1.5, 2.5, -2.5, 127.5, -127.5, 1e6, -1e6, 0.0]) / 2048.0
    h8, l8 = C.int8_planes(hi, lo, 1.0)
    assert h8.tolist() == [0, 2, 2, 0, -2, 126, 127, 127, -127]
    assert l8.tolist() == [0, 2, 2, -2, 127, -127, 127, -127, 0]


def test_t_row_scale_is_the_kernels_bit_trick():
    """the smallest power of two >= amax / 127 (exact arithmetic) == (bits(f32(amax f32(1 / 127))) + 0x007fffff) & 0x7f800000 for every
    positive finite f16 amax; 127 x 2^j gives 2^j, the next f16 above it 2^(j + 1); an all-zero row 1.0"""
    amax = np.arange(1, 0x7c00, dtype=np.uint16).view(np.float16).astype(np.float32)
    assert (C.t_row_scale(amax) == C.t_row_scale_bits(amax)).all()
    assert C.t_row_scale(0.0) == 1.0 and C.t_row_scale_bits(np.float32(0.0)) == 1.0
    for j in range(-14, 9):
        a = np.float16(127.0 * 2.0 ** j)
        assert C.t_row_scale(a) == 2.0 ** j and C.t_row_scale(np.nextafter(a, np.float16(np.inf))) == 2.0 ** (j + 1)


def test_tie_values():
    m = np.float32(np.float32(1024.0) * np.float32(C.LOG2E))
    t = C.tie_values(m)
    assert len(t) == 3072 and (C.f16_once(t, m) != C.f16_twice(t, m)).sum() == 514
    assert (C.f16_once(t[:514], m) != C.f16_twice(t[:514], m)).all()


def test_t_case_rows_hit_the_scale_boundaries():
    segs, ldt = C.t_case_segments([200, 100, 52])
    T = C.t_case_rows(np.random.default_rng(0), 14, segs, ldt, 10)
    body, written = C.t_row_bytes(T, segs, [1024.0] * 3, mx6=False)
    sc = body[:, -32:].view(np.float32)[:, :3]
    assert (sc[1] == 1.0).all() and (sc[2] == 8.0).all() and (sc[3] == 16.0).all() and (sc[4] < 2.0 ** -25).all()
    assert written[:, :-32].all() and written[:, -32:-20].all() and not written[:, -20:].any()


def test_tm_image_index_is_the_documented_placement():
    ld_tm, R = C.t_stride([(200, 0, 7), (100, 200, 4), (52, 300, 2)]), 40
    idx = C.tm_image_index(R, ld_tm)
    for r, g in ((0, 0), (5, 3), (31, 103), (33, 17)):
        assert idx[r, 16 * g + 7] == (r // 32) * 32 * ld_tm * 4 + g * 512 + (r % 32) * 16 + 7
    assert idx[33, 4 * ld_tm - 32 + 4 * 2] == 32 * ld_tm * 4 + 32 * (ld_tm * 4 - 32) + 1 * 32 + 4 * 2


@pytest.mark.parametrize("k", C.SPLIT_K)
@pytest.mark.parametrize("rows", C.SPLIT_ROWS)
def test_pack_split_f16(rows, k):
    C.run_pack_split(FK, MEM, rows, k)


def test_pack_split_f16_scale_that_is_no_power_of_two():
    C.run_pack_split_ties(FK, MEM)


@pytest.mark.parametrize("rows", C.COL_ROWS)
def test_pack_split_f16_col(rows):
    C.run_pack_split_col(FK, MEM, rows)


@pytest.mark.parametrize("k", C.DEQUANT_K)
@pytest.mark.parametrize("n_codes", C.DEQUANT_CODES)
def test_dequant_u8(n_codes, k):
    C.run_dequant_u8(FK, MEM, n_codes, k)


@pytest.mark.parametrize("mx6", [False, True], ids=["int8", "mx6"])
@pytest.mark.parametrize("k", C.MIXED_K)
@pytest.mark.parametrize("rows", C.MIXED_ROWS)
def test_pack_mixed(rows, k, mx6):
    C.run_pack_mixed(FK, MEM, rows, k, mx6)


@pytest.mark.parametrize("R", C.T_ROWS)
@pytest.mark.parametrize("widths", C.T_WIDTHS, ids=lambda w: "-".join(map(str, w)))
def test_pack_t_mixed_and_mixed6(widths, R):
    """FakeLib.jlm_pack_t_mixed: the f16 plane, the int8 hi plane and the row maximum from ONE rounding of the exact product T (2^eT log2 e), as
    pack_t_mixed_kernel has them; FakeLib.jlm_pack_t_mixed6 from the f32 product, as pack_t_mx6_kernel"""
    C.run_pack_t(FK, MEM, widths, R)


def test_split_bias_correction_undoes_the_held_constant():
    """the bias column of split rows meets f32(t_scale log2 e) as f16 hi + lo: the correction times that constant is t_scale log2 e"""
    from jlm_amd.rowformats import LOG2E, split_bias_correction
    for e in (-3, 0, 5, 9, 11):
        ts = 2.0 ** e
        x = np.float32(np.float32(ts) * np.float32(LOG2E))
        hi = np.float16(x)
        held = float(hi) + float(np.float16(x - np.float32(hi)))
        c = split_bias_correction(ts)
        assert abs(held * c / (ts * LOG2E) - 1.0) <= 1e-15
        assert abs((1.0 / c - 1.0) - 6.928e-8) <= 1e-10            # log2 e in 22 bits: the same at every power-of-two scale
