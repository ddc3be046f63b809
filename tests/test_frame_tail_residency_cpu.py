"""CPU-only: the register / scratch / LDS budget of the fused frame tail (frame_tail_mx6_kernel, csrc/jlm_frame_tail.hip), read from the
gfx950 code object inside the BUILT library like tests/test_kernel_residency_cpu.py reads the other kernels of the frame.

The kernel is launched with one workgroup per cell behind the T projection; its budget -- 64 allocated registers, no scratch, at most
32 KB of LDS at the headline row stride (ldt = 352, beam <= 16) -- is what a resident normaliser workgroup leaves free on a CU
(DESIGN.md 4.1), so a fused tail of another batch in flight can be placed beside it.  `pytest -s` prints the line."""
import ctypes
import os

import pytest

from jlm_amd import _lib
from tests.test_kernel_residency_cpu import CU_LDS, NORMALISER, SIMD_REGS, _alloc, _kernel_table, _one

KERNEL = "frame_tail_mx6_kernelE"
HEADLINE_LDT = 352           # BASELINE configs[1]: D-softmax* 200 + 100 + 50 = 350 columns of T, rows padded to 16 bytes


@pytest.fixture(scope="module")
def table():
    assert os.path.exists(_lib.LIB_PATH), "libjlm_hip.so is not built (python __graft_entry__.py)"
    return _kernel_table(_lib.LIB_PATH)


def _lds(ldt):
    lib = ctypes.CDLL(_lib.LIB_PATH)             # a pure host function: no GPU needed
    lib.jlm_pack_edge_mx6_lds_bytes.argtypes = [ctypes.c_int]
    return lib.jlm_pack_edge_mx6_lds_bytes(ldt)


def test_frame_tail_fits_64_registers_without_scratch(table):
    k = _one(table, KERNEL)
    print("\n%-24s vgpr %3d -> %3d allocated, agpr %d, scratch %d, sgpr spills %d, LDS static %d + dynamic %d" % (
        "frame_tail_mx6_kernel", k["vgpr_count"], _alloc(k["vgpr_count"]), k["agpr_count"], k["private_segment_fixed_size"],
        k["sgpr_spill_count"], k["group_segment_fixed_size"], _lds(HEADLINE_LDT)))
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, "scratch: the kernel spills"
    assert _alloc(k["vgpr_count"] + k["agpr_count"]) <= 64
    # ... which is what two resident normaliser waves per SIMD leave
    assert _alloc(k["vgpr_count"]) + 2 * _alloc(_one(table, NORMALISER)["vgpr_count"]) <= SIMD_REGS


def test_frame_tail_lds_at_the_headline_shape(table):
    k = _one(table, KERNEL)
    lds = _lds(HEADLINE_LDT)
    assert lds >= 16 * HEADLINE_LDT * 4                # sixteen rows (beam <= 16) of the cell
    assert k["group_segment_fixed_size"] + lds <= 32 * 1024
    assert k["group_segment_fixed_size"] + lds + 128 * 1024 <= CU_LDS       # beside the normaliser's 128 KB
    assert _lds(350) == -1                             # a row stride that is no multiple of 4 floats is refused
