// The operand decode of the cache's dot products, shared by cache_query_kernel (csrc/jlm_cache_mix.hip) and cache_cell_query_kernel
// (csrc/jlm_cache_edge.hip): both give the same bits for the same (query row, key row, theta).
#pragma once
#include "jlm_common.h"

namespace {

union Rec {
    uint4 u;
    f16x8 h;
    float f[4];
};

// the eight values of one 32-byte unit: split rows f32(hi) + f32(lo) (the scale stays in, theta carries 1 / h_scale^2), else the f32s
template <bool SPLIT>
__device__ __forceinline__ void cq_unit(const uint4 *row, int u, float v[8]) {
    Rec a, b;
    a.u = row[2 * u];
    b.u = row[2 * u + 1];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = SPLIT ? (float)a.h[i] + (float)b.h[i] : (i < 4 ? a.f[i] : b.f[i - 4]);
}

}  // namespace
