// The log-normaliser of one row of materialised f32 logits: the ONE definition of the arithmetic behind topk_rows_kernel's nll
// (csrc/jlm_topk.hip), shared with the kernels that patch a row relative to it -- cache_mix_rows_kernel (csrc/jlm_cache_mix.hip) and
// ngram_mix_rows_kernel (csrc/jlm_ngram_mix.hip) -- so that the L they add is the L the top-k, rank and completion kernels subtract.
//
// One workgroup of RL_WAVES waves per row.  The row is read as 16-byte chunks (4 words); an "iteration" is 64 consecutive chunks, one
// per lane, and wave w owns the contiguous iterations [w ipw, (w + 1) ipw).  Per lane a running maximum m and an f64 sum s of f32
// expf(y - m), rescaled by exp(m_old - m_new) in f64 when a group of RL_GROUP chunks raises the maximum; an xor tree over the wave;
// the waves merged in order.  A lane that has only seen -inf or NaN keeps m = -inf and sums expf(y - 0) (0, or NaN for a NaN).
// lse = M + log S.  topk_row calls the pieces on the chunks it has loaded for its candidate lists; the mix kernels call rl_row.
// (sample_rows_kernel and rank_rows_kernel sum in orders of their own: nothing claims they equal this one to the bit.)
#pragma once
#include "jlm_common.h"

#define RL_WAVES 4                      // waves a row's workgroup has: every caller asserts its thread count against it
#define RL_GROUP 4                      // chunks a lane takes per trip: the running maximum moves by groups of this many

// a partial sum taken relative to max m, relative to M >= m.  m = -inf: nothing finite was summed, the sum is 0 (or NaN after a NaN
// logit) and stays as it is -- exp(-inf - -inf) would turn an empty lane's or wave's 0 into NaN.
__device__ __forceinline__ double rl_rescale(double s, float m, float M) { return m > -INFINITY ? s * exp((double)m - (double)M) : s; }

// one lane's group: chunks v[u] of iterations it + u (chunk (it + u) * 64 + lane), words at or past n_cols left out, into (m, s)
__device__ __forceinline__ void rl_group(const f32x4 (&v)[RL_GROUP], int it, int lane, int n_cols, float &m, double &s) {
    float cm = -INFINITY;
#pragma unroll
    for (int u = 0; u < RL_GROUP; ++u)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (4 * ((it + u) * 64 + lane) + j < n_cols) cm = fmaxf(cm, v[u][j]);
    if (cm > m) { s = rl_rescale(s, m, cm); m = cm; }
    const float me = m > -INFINITY ? m : 0.0f;
#pragma unroll
    for (int u = 0; u < RL_GROUP; ++u)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (4 * ((it + u) * 64 + lane) + j < n_cols) s += (double)expf(v[u][j] - me);
}

// the 64 lanes' (m, s) -> the wave's, on every lane
__device__ __forceinline__ void rl_wave_merge(float &m, double &s) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float m2 = __shfl_xor(m, off);
        const double s2 = __shfl_xor(s, off);
        const float M = fmaxf(m, m2);
        s = rl_rescale(s, m, M) + rl_rescale(s2, m2, M);
        m = M;
    }
}

// the waves' (s_m[w], s_s[w]) -> the row's (M, S), the waves in order
__device__ __forceinline__ void rl_block_merge(const float *s_m, const double *s_s, float &M, double &S) {
    M = s_m[0];
    for (int w = 1; w < RL_WAVES; ++w) M = fmaxf(M, s_m[w]);
    S = 0.0;
    for (int w = 0; w < RL_WAVES; ++w) S += rl_rescale(s_s[w], s_m[w], M);
}

// the whole row -> (M, S) on every thread of its workgroup (64 * RL_WAVES threads, all of them call); s_m, s_s: RL_WAVES entries of LDS
__device__ __forceinline__ void rl_row(const f32x4 *__restrict__ row, int n_cols, float *s_m, double *s_s, float &M, double &S) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int n4 = (n_cols + 3) >> 2, n_it = (n4 + 63) >> 6;
    const int ipw = (n_it + RL_WAVES - 1) / RL_WAVES;
    const int it0 = wv * ipw, it1 = min(it0 + ipw, n_it);
    float m = -INFINITY;
    double s = 0.0;
    for (int it = it0; it < it1; it += RL_GROUP) {
        f32x4 v[RL_GROUP];
#pragma unroll
        for (int u = 0; u < RL_GROUP; ++u) {
            const int c = (it + u) * 64 + lane;
            v[u] = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
            if (it + u < it1 && c < n4) v[u] = row[c];
        }
        rl_group(v, it, lane, n_cols, m, s);
    }
    rl_wave_merge(m, s);
    if (lane == 0) { s_m[wv] = m; s_s[wv] = s; }
    __syncthreads();                                               // (every read of the row is behind this barrier)
    rl_block_merge(s_m, s_s, M, S);
}
