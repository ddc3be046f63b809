// jlm_cache.hip -- the continuous cache of teacher-forced scoring (include/jlm_hip.h jlm_cache_rows):
// cache_rows_kernel, a banded, causal H.H^T over a ring of state rows with a word-match mask where attention has a value matrix.
//
// One workgroup per (row, block of 32 queries), 8 waves.  The scores come off the matrix pipe TRANSPOSED -- keys are the MFMA rows,
// queries the MFMA columns -- so that a lane owns one query (its column) and sixteen keys of a 32-key tile (its accumulator
// registers): the running maximum and the two sums of a query live in that lane's registers and nothing crosses lanes inside the
// key loop.  Wave w takes the tile pairs w, w + 8, ...; both tiles of a pair multiply against one load of the query fragments.
// Split rows ([8 hi][8 lo] f16, the LSTM step's own output): three v_mfma_f32_32x32x16_f16 per 16 k over the stored halves
// (hi.hi + hi.lo + lo.hi), 1 / h_scale^2 folded into theta on the host.  f32 rows: v_mfma_f32_32x32x2_f32, a k-ordered
// fmaf chain -- no split on load: the pass is a stream over the ring, and the exact pipe gives the f32 rows the plain gamma_H bound.
// At the end the sixteen partial states of a query (two half-waves x eight waves) are folded in a fixed order and lane n of the
// first wave(s) writes log M - log Z.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/jlm_hip.h"

namespace {

constexpr int CQ = 32;                 // queries per workgroup: the MFMA columns
constexpr int CK = 32;                 // keys per tile: the MFMA rows
constexpr int CW = 8;                  // waves per workgroup
constexpr int KT = 2;                  // key tiles per load of the query fragments

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

struct CacheArgs {
    const uint4 *hist;
    const int *words, *first, *len;
    float *lpc;
    int *flags;
    int cap, n_rows, H, pos0, n_query, N, n_theta;
    float theta[JLM_CACHE_MAX_THETAS];          // split rows: theta / h_scale^2
};

union Frag {
    uint4 u;
    f16x8 h;
    float f[4];
};

// the state of one query's online sums in one lane: the running maximum m of its scores so far, Z = sum exp(s - m), M = the same sum
// over the keys whose word matches
struct Online {
    float m, Z, M;
};

template <bool SPLIT>
__global__ void __launch_bounds__(CW * 64) cache_rows_kernel(const CacheArgs a) {
    __shared__ float red[JLM_CACHE_MAX_THETAS][CW][3][CQ];
    const int r = blockIdx.y, q_lo = blockIdx.x * CQ;
    const int n_q_row = min(a.len[r], a.n_query);
    if (q_lo >= n_q_row) return;                                   // (uniform: rows >= len and their lpc are left alone)
    const int nq = min(CQ, n_q_row - q_lo);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int col = lane & 31, half = lane >> 5;
    const int qpos0 = a.pos0 + q_lo;                               // position of the block's first query
    const int k_lo = max(max(qpos0 - a.N, a.first[r]), 0);         // oldest key any query of the block sees
    const int k_hi = qpos0 + nq - 1;                               // keys are < the block's last query
    const int n_keys = k_hi - k_lo;
    const size_t row4 = (size_t)a.H / 4;                           // 16-byte records of a state row
    const size_t slot4 = (size_t)a.n_rows * row4;

    // this lane's query: column `col`
    const bool q_ok = col < nq;
    const int qp = qpos0 + col;
    const int q_slot = qp % a.cap;
    const uint4 *q_row = a.hist + (size_t)q_slot * slot4 + (size_t)r * row4;
    const int q_word = q_ok ? a.words[(size_t)q_slot * a.n_rows + r] : 0;

    Online st[JLM_CACHE_MAX_THETAS];
#pragma unroll
    for (int t = 0; t < JLM_CACHE_MAX_THETAS; ++t) st[t] = Online{-INFINITY, 0.0f, 0.0f};
    bool bad = false;

    for (int tp = w; tp * (KT * CK) < n_keys; tp += CW) {
        // this lane's key row of each tile of the pair: MFMA row `col`
        const uint4 *k_row[KT];
        bool k_ok[KT];
#pragma unroll
        for (int i = 0; i < KT; ++i) {
            const int kp = k_lo + (tp * KT + i) * CK + col;
            k_ok[i] = kp < k_hi;
            k_row[i] = a.hist + (size_t)((k_ok[i] ? kp : k_lo) % a.cap) * slot4 + (size_t)r * row4;
        }
        f32x16 acc[KT];
#pragma unroll
        for (int i = 0; i < KT; ++i)
#pragma unroll
            for (int j = 0; j < 16; ++j) acc[i][j] = 0.0f;
        const uint4 zero = make_uint4(0, 0, 0, 0);
        if (SPLIT) {
            // 16 k per step: lane (row, half) holds k = 16 kb + 8 half .. + 7 -- block 2 kb + half of the row, [8 hi][8 lo]
            for (int kb = 0; kb < a.H / 16; ++kb) {
                const int rec = (2 * kb + half) * 2;
                Frag bh, bl;
                bh.u = q_ok ? q_row[rec] : zero;
                bl.u = q_ok ? q_row[rec + 1] : zero;
#pragma unroll
                for (int i = 0; i < KT; ++i) {
                    Frag ah, al;
                    ah.u = k_ok[i] ? k_row[i][rec] : zero;
                    al.u = k_ok[i] ? k_row[i][rec + 1] : zero;
                    acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah.h, bh.h, acc[i], 0, 0, 0);
                    acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah.h, bl.h, acc[i], 0, 0, 0);
                    acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al.h, bh.h, acc[i], 0, 0, 0);
                }
            }
        } else {
            // 8 k per step, four MFMAs of 2 k: lane (row, half) loads k = 8 c + 4 half .. + 3, and MFMA j sums k = 8 c + j and 8 c + 4 + j
            for (int c = 0; c < a.H / 8; ++c) {
                const int rec = 2 * c + half;
                Frag b;
                b.u = q_ok ? q_row[rec] : zero;
#pragma unroll
                for (int i = 0; i < KT; ++i) {
                    Frag k;
                    k.u = k_ok[i] ? k_row[i][rec] : zero;
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(k.f[j], b.f[j], acc[i], 0, 0, 0);
                }
            }
        }
        // accumulator register j of tile i: key row (j & 3) + 8 (j >> 2) + 4 half, query column col
#pragma unroll
        for (int i = 0; i < KT; ++i) {
            const int base = k_lo + (tp * KT + i) * CK + 4 * half;
            unsigned ok = 0, match = 0;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int kp = base + (j & 3) + 8 * (j >> 2);
                // the causal and window mask: max(q - N, first) <= i < q  (kp >= k_lo >= first)
                const bool v = q_ok && kp < qp && kp >= qp - a.N;
                if (v) {
                    ok |= 1u << j;
                    if (a.words[(size_t)(kp % a.cap) * a.n_rows + r] == q_word) match |= 1u << j;
                    if (!isfinite(acc[i][j])) bad = true;
                }
            }
#pragma unroll
            for (int t = 0; t < JLM_CACHE_MAX_THETAS; ++t) {
                if (!ok || t >= a.n_theta) continue;               // (uniform in t; no break: the loop must unroll, st[] stays in registers)
                const float th = a.theta[t];
                float s[16], mx = st[t].m;
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    s[j] = th * acc[i][j];
                    if (ok >> j & 1) mx = fmaxf(mx, s[j]);
                }
                const float scale = expf(st[t].m - mx);            // (m = -inf at first: 0, and Z = M = 0 then)
                float Z = st[t].Z * scale, M = st[t].M * scale;
#pragma unroll
                for (int j = 0; j < 16; ++j)
                    if (ok >> j & 1) {
                        const float e = expf(s[j] - mx);
                        Z += e;
                        if (match >> j & 1) M += e;
                    }
                st[t] = Online{mx, Z, M};
            }
        }
    }
    if (bad && a.flags) atomicOr(a.flags, 1);

    // fold: the two half-waves of a wave through a lane exchange, then the eight waves through LDS, in a fixed order
#pragma unroll
    for (int t = 0; t < JLM_CACHE_MAX_THETAS; ++t) {
        if (t >= a.n_theta) continue;
        const float m2 = __shfl_xor(st[t].m, 32), Z2 = __shfl_xor(st[t].Z, 32), M2 = __shfl_xor(st[t].M, 32);
        // (half 0 first on both sides, so that the two lanes of a query hold the same bits)
        const float ma = half ? m2 : st[t].m, Za = half ? Z2 : st[t].Z, Ma = half ? M2 : st[t].M;
        const float mb = half ? st[t].m : m2, Zb = half ? st[t].Z : Z2, Mb = half ? st[t].M : M2;
        const float mx = fmaxf(ma, mb);
        float Z = 0.0f, M = 0.0f;
        if (mx > -INFINITY) {
            const float ea = expf(ma - mx), eb = expf(mb - mx);
            Z = Za * ea + Zb * eb;
            M = Ma * ea + Mb * eb;
        }
        if (half == 0) {
            red[t][w][0][col] = mx;
            red[t][w][1][col] = Z;
            red[t][w][2][col] = M;
        }
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < a.n_theta * CQ; idx += CW * 64) {
        const int t = idx / CQ, n = idx % CQ;
        if (n >= nq) continue;
        float mx = -INFINITY;
        for (int i = 0; i < CW; ++i) mx = fmaxf(mx, red[t][i][0][n]);
        float out = -INFINITY;                                     // no entry at all (n_q = 0): defined as -inf, unused
        if (mx > -INFINITY) {
            float Z = 0.0f, M = 0.0f;
            for (int i = 0; i < CW; ++i) {
                const float e = expf(red[t][i][0][n] - mx);      // (a wave without a key: exp(-inf) = 0)
                Z += red[t][i][1][n] * e;
                M += red[t][i][2][n] * e;
            }
            out = logf(M) - logf(Z);                            // (no match: log 0 = -inf exactly)
        }
        a.lpc[((size_t)t * a.n_query + (q_lo + n)) * a.n_rows + r] = out;
    }
}

// the copy behind a scoring step (jlm_score_cache_frames): the live rows of the state set the step wrote, contiguous, into their ring slot,
// 16 bytes a lane, and the step's targets into the word ring -- one launch where two copy calls cost more host time than the step's kernels
__global__ void __launch_bounds__(256) cache_store_kernel(const uint4 *__restrict__ src, uint4 *__restrict__ dst, const int *__restrict__ target,
                                                          int *__restrict__ words, int n4, int bound) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n4) dst[i] = src[i];
    if (i < bound) words[i] = target[i];
}

}  // namespace

// rows 0 .. bound - 1 of h_rows [.., H] (4-byte values, 16-byte aligned) -> hist_slot, target[0 .. bound) -> words_slot; asynchronous, on `stream`
int jlm_cache_store(const void *h_rows, const int *target, int bound, int H, void *hist_slot, int *words_slot, void *stream) {
    if (bound <= 0) return 0;
    if (H <= 0 || H % 4 != 0 || (long long)bound * (H / 4) > 0x7fffff00ll) return -1;
    if ((((uintptr_t)h_rows | (uintptr_t)hist_slot) & 15) != 0) return -1;
    const int n4 = bound * (H / 4);
    cache_store_kernel<<<dim3((n4 + 255) / 256), dim3(256), 0, (hipStream_t)stream>>>((const uint4 *)h_rows, (uint4 *)hist_slot, target, words_slot, n4,
                                                                                     bound);
    return (int)hipGetLastError();
}

// the launcher's refusals on their own (jlm_score_cache_frames asks before its first launch): -1, or 0
int jlm_cache_refuse(const void *hist, const int *words, int cap, int n_rows, int H, int split, float h_scale, int pos0, int n_query,
                     const int *first, const int *len, int N, const float *thetas, int n_theta, const float *lpc) {
    if (n_rows < 0 || n_query < 0 || N < 1 || cap < 1 || pos0 < 0) return -1;
    if ((long long)N + n_query > cap) return -1;
    if ((long long)pos0 + n_query + cap > 0x7fffffffll) return -1;
    if (H <= 0 || H % 32 != 0) return -1;                          // what jlm_lstm_step / jlm_lstm_step_xg accept
    if (n_theta < 1 || n_theta > JLM_CACHE_MAX_THETAS || !thetas) return -1;
    for (int t = 0; t < n_theta; ++t)
        if (!(thetas[t] >= 0.0f) || !isfinite(thetas[t])) return -1;
    if (split && !(h_scale > 0.0f && isfinite(h_scale))) return -1;
    if (n_rows == 0 || n_query == 0) return 0;
    if (n_rows > 65535) return -1;
    if (!hist || !words || !first || !len || !lpc) return -1;
    if (((uintptr_t)hist & 15) != 0 || (((uintptr_t)words | (uintptr_t)first | (uintptr_t)len | (uintptr_t)lpc) & 3) != 0) return -1;
    return 0;
}

extern "C" int jlm_cache_rows(const void *hist, const int *words, int cap, int n_rows, int H, int split, float h_scale, int pos0,
                              int n_query, const int *first, const int *len, int N, const float *thetas, int n_theta, float *lpc,
                              int *flags, void *stream) {
    if (int rc = jlm_cache_refuse(hist, words, cap, n_rows, H, split, h_scale, pos0, n_query, first, len, N, thetas, n_theta, lpc)) return rc;
    if (n_rows == 0 || n_query == 0) return 0;
    if (flags && ((uintptr_t)flags & 3) != 0) return -1;
    CacheArgs a;
    a.hist = (const uint4 *)hist; a.words = words; a.first = first; a.len = len; a.lpc = lpc; a.flags = flags;
    a.cap = cap; a.n_rows = n_rows; a.H = H; a.pos0 = pos0; a.n_query = n_query; a.N = N; a.n_theta = n_theta;
    for (int t = 0; t < JLM_CACHE_MAX_THETAS; ++t)
        a.theta[t] = t < n_theta ? (split ? thetas[t] / (h_scale * h_scale) : thetas[t]) : 0.0f;
    const dim3 grid((n_query + CQ - 1) / CQ, n_rows);
    if (split)
        cache_rows_kernel<true><<<grid, dim3(CW * 64), 0, (hipStream_t)stream>>>(a);
    else
        cache_rows_kernel<false><<<grid, dim3(CW * 64), 0, (hipStream_t)stream>>>(a);
    return (int)hipGetLastError();
}
