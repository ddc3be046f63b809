"""GPU: every kernel that WRITES one of the packed operand formats (include/jlm_hip.h: split-f16 rows, int8 "mixed" rows, mx6 rows) against
the format's exact definition in tests/operand_cases.py -- numpy, float64 products rounded once -- byte for byte: destinations are
pre-filled with a sentinel, the written region is compared with the definition and everything else with the sentinel; no tolerance and no
excused element.  The rest of the GPU suite packs its inputs with these kernels and hands the device-made bytes to the numpy restatement
(tests/fake_hip.py), so a packer that is subtly wrong is wrong on both sides there; tests/test_operand_formats_cpu.py holds the restatement
to the same definitions on the same cases.

jlm_pack_split_f16 (csrc/jlm_split.hip pack_split_kernel, jlm_common.h jlm_split2), jlm_pack_split_f16_col, jlm_dequant_u8,
jlm_pack_mixed in both forms (csrc/jlm_mixed.hip pack_mixed_kernel / pack_mx6_kernel), jlm_pack_t_mixed / jlm_pack_t_mixed6
(pack_t_mixed_kernel / pack_t_mx6_kernel).  The split-row epilogue of the LSTM step: tests/test_gpu_gate_forms.py."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
from jlm_amd import _lib                 # noqa: E402
from tests import operand_cases as C     # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    lib = _lib.lib()
    buf = ctypes.create_string_buffer(128)
    assert lib.jlm_device_arch(0, buf, 128) == 0
    assert buf.value.decode().startswith("gfx950"), buf.value
    return lib


class DevMem:
    """buffers on the device; packed hypothesis rows come back granule-major (operand_cases.tm_image_index)"""
    granule_major = True

    @property
    def stream(self):
        return torch.cuda.current_stream().cuda_stream

    @staticmethod
    def put(a):
        return torch.as_tensor(np.array(a, copy=True, order="C")).cuda()

    @staticmethod
    def ptr(h, off=0):
        return h.data_ptr() + off

    @staticmethod
    def get(h):
        torch.cuda.synchronize()
        return h.cpu().numpy().reshape(-1).view(np.uint8)


MEM = DevMem()


@pytest.mark.parametrize("k", C.SPLIT_K)
@pytest.mark.parametrize("rows", C.SPLIT_ROWS)
def test_pack_split_f16(L, rows, k):
    """rows x blocks straddle the 256 threads of a workgroup; ld = k and a column-offset view; ld_dst = pad16(k) and 32 more (untouched);
    k .. pad16(k) zero; N(0, 1) with +-0, f16-subnormal hi, f16-subnormal lo, +-65504 / scale and f16 rounding ties at scales 2^-3, 2^10, 2^14"""
    C.run_pack_split(L, MEM, rows, k)


def test_pack_split_f16_scale_that_is_no_power_of_two(L):
    """jlm_split2 pins the scaled value and hi in registers so that hi and lo are taken from the SAME f32 product; on inputs whose f32
    product is an f16 tie while the exact product is not, a conversion fused into one of the two uses shows as hundreds of wrong bytes"""
    C.run_pack_split_ties(L, MEM)


@pytest.mark.parametrize("rows", C.COL_ROWS)
def test_pack_split_f16_col(L, rows):
    C.run_pack_split_col(L, MEM, rows)


@pytest.mark.parametrize("k", C.DEQUANT_K)
@pytest.mark.parametrize("n_codes", C.DEQUANT_CODES)
def test_dequant_u8(L, n_codes, k):
    """codebook entries -0.0, a subnormal, inf and NaNs with payloads are copied bit for bit; codes >= n_codes give +0.0"""
    C.run_dequant_u8(L, MEM, n_codes, k)


@pytest.mark.parametrize("mx6", [False, True], ids=["int8", "mx6"])
@pytest.mark.parametrize("k", C.MIXED_K)
@pytest.mark.parametrize("rows", C.MIXED_ROWS)
def test_pack_mixed(L, rows, k, mx6):
    """quotients on .5 (ties to even), planes that clip at +-127 (and an s8 one power of two too small), zero planes behind k, the two
    bias columns with a bias and without, rows that have no room for them (ld_dst = k)"""
    C.run_pack_mixed(L, MEM, rows, k, mx6)


@pytest.mark.parametrize("R", C.T_ROWS)
@pytest.mark.parametrize("widths", C.T_WIDTHS, ids=lambda w: "-".join(map(str, w)))
def test_pack_t_mixed_and_mixed6(L, widths, R):
    """tie rows, an all-zero row (scale 1.0), largest |hi| exactly 127 x 8 (scale 8) and the next f16 above (16), a row x 2^-30, alternating
    zeros; the per-segment scale floats, the granule placement, the bias constants; rows from n_dev on and the rest of the 32-row image keep
    the sentinel.  The int8 form shows the ONCE-rounded f16 plane, the mx6 form the twice-rounded one, and on the tie rows they differ."""
    C.run_pack_t(L, MEM, widths, R)
