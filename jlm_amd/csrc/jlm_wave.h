// Wave-wide (64 lanes) reductions shared by kernels that must agree on their result: the beam step's selection rounds
// (csrc/jlm_beam.hip) and tail_predict_kernel's tp_select (csrc/jlm_tail.hip).
#pragma once
#include "jlm_common.h"

// Wave-wide lexicographic minimum of (v, i), result in every lane.  DPP cross-lane moves (a few
// cycles each) instead of __shfl_xor, which is ds_bpermute on this ISA: three dependent LDS-crossbar
// round trips per step made one selection round 0.9 us (8.8 of the kernel's 19 us for beam = 10).
// Mirror steps leave every lane of a 16-lane row with the row's minimum; row_bcast15 / 31 carry it to
// the last row; lane 63 holds the wave's and is read back through SGPRs.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ void argmin_dpp_step(double &v, int &i) {
    const int lo = __double2loint(v), hi = __double2hiint(v);
    const int lo2 = __builtin_amdgcn_update_dpp(lo, lo, CTRL, ROW_MASK, 0xf, false);
    const int hi2 = __builtin_amdgcn_update_dpp(hi, hi, CTRL, ROW_MASK, 0xf, false);
    const int i2 = __builtin_amdgcn_update_dpp(i, i, CTRL, ROW_MASK, 0xf, false);
    const double v2 = __hiloint2double(hi2, lo2);
    if (v2 < v || (v2 == v && i2 < i)) { v = v2; i = i2; }
}
__device__ __forceinline__ void wave_argmin(double &v, int &i) {
    argmin_dpp_step<0xB1, 0xf>(v, i);      // quad_perm(1,0,3,2)
    argmin_dpp_step<0x4E, 0xf>(v, i);      // quad_perm(2,3,0,1)
    argmin_dpp_step<0x141, 0xf>(v, i);     // row_half_mirror
    argmin_dpp_step<0x140, 0xf>(v, i);     // row_mirror
    argmin_dpp_step<0x142, 0xa>(v, i);     // row_bcast15 into rows 1 and 3
    argmin_dpp_step<0x143, 0xc>(v, i);     // row_bcast31 into rows 2 and 3
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), 63);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), 63);
    i = __builtin_amdgcn_readlane(i, 63);
    v = __hiloint2double(hi, lo);
}
