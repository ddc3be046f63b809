// jlm_memory_topk.hip -- exact top-K retrieval over a memory of hidden states (include/jlm_hip.h jlm_memory_topk):
// for every live query row, the min(K, N) entries of the memory that come first in the order "larger s_i = theta (h_q . k_i) first,
// smaller i first among equal bits", best first, in the layout jlm_cache_mix_rows reads a window in.
//
// The launcher walks the memory in chunks of C keys (C a multiple of 32, sized from the workspace) and launches, per chunk, two kernels:
//
// memory_topk_score_kernel   memory_rows_kernel's products (csrc/jlm_memory.hip: keys are the MFMA rows, queries the MFMA columns, the
//                            same instructions in the same k order, restated below), on the grid (block of 32 queries) x (range of 512
//                            keys of the chunk); wave w of a workgroup takes the tile pair w of its range.  A lane's sixteen
//                            accumulators of a tile are four runs of four consecutive keys of ONE query: each run leaves as one 16-byte
//                            store into the chunk's score array [row][C] of the workspace.  No online sums, nothing crosses lanes.
// memory_topk_select_kernel  one workgroup per live row.  Every (score, index) pair is ONE 56-bit integer, the order-preserving image
//                            of the score's bits above the complement of the 24-bit index, so that the total order of the definition
//                            is the integer order and no two entries are equal.  A radix select (LDS histograms of 256 bins, a byte
//                            a pass from the top, integer counts only) finds the min(K, chunk)-th largest composite of the chunk
//                            exactly; the entries at or above it are gathered into LDS (their slots come from an integer counter:
//                            the SET is determined, its order is not), the running list of the earlier chunks is appended, a bitonic
//                            sort of at most 2 K composites orders them, and the first min(K, keys so far) are the new running list
//                            -- in the workspace, or, behind the last chunk, decoded into s / ret_words / ret_idx.
//
// What a row's result depends on: its own state row, the memory, theta, K.  An MFMA column is a function of its own B operand and the A
// rows; the select reads nothing but its row's scores of this chunk and its row's running list, both written by this call; a set of
// distinct integers has one sorted order, so neither the chunk size nor the completion order of the LDS counters enters.
// Plain vector stores to global memory, one writer per address; the only global atomic is the OR on the flag word.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/jlm_hip.h"

namespace {

constexpr int CQ = 32;                 // queries per workgroup of the score kernel: the MFMA columns
constexpr int CK = 32;                 // keys per tile: the MFMA rows
constexpr int CW = 8;                  // waves per workgroup of the score kernel
constexpr int KT = 2;                  // key tiles per load of the query fragments
constexpr int WG_KEYS = CW * KT * CK;  // keys a workgroup of the score kernel covers: 512
constexpr int ST = 256;                // threads of a select workgroup
constexpr int KMAX = JLM_MEMORY_TOPK_MAX;

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

union Frag {
    uint4 u;
    f16x8 h;
    float f[4];
};

struct TopkArgs {
    const uint4 *keys, *q_rows;
    const int *key_words, *n_dev;
    float *scores;                              // workspace: [n_rows_max][C] f32, the chunk's scores
    unsigned long long *run;                    // workspace: [n_rows_max][K] composites, the running list
    float *s;
    int *ret_words, *ret_idx, *flags;
    int N, H, C, K, n_rows_max, n_rows, ld_s;
    int c0, len, last;                          // this chunk: keys c0 <= i < c0 + len; last != 0: write the outputs
    float theta;                                // split rows: theta / h_scale^2
};

__device__ inline int live_rows(const TopkArgs &a) {
    int n = a.n_rows_max;
    if (a.n_dev) n = max(0, min(n, *a.n_dev));
    return n;
}

template <bool SPLIT>
__global__ void __launch_bounds__(CW * 64) memory_topk_score_kernel(const TopkArgs a) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int col = lane & 31, half = lane >> 5;
    const int q = blockIdx.x * CQ + col;
    const bool q_ok = q < live_rows(a);
    const int t_lo = blockIdx.y * WG_KEYS + w * (KT * CK);         // this wave's tile pair, as an offset into the chunk
    if (t_lo >= a.len || __ballot(q_ok) == 0) return;              // (wave-uniform; the kernel has no barrier)
    const int k_hi = a.c0 + a.len;
    const size_t row4 = (size_t)a.H / 4;                           // 16-byte records of a state row
    const uint4 *q_row = a.q_rows + (size_t)(q_ok ? q : 0) * row4;

    const uint4 *k_row[KT];
    bool k_ok[KT];
#pragma unroll
    for (int i = 0; i < KT; ++i) {
        const int kp = a.c0 + t_lo + i * CK + col;                 // this lane's key row of tile i: MFMA row `col`
        k_ok[i] = kp < k_hi;
        k_row[i] = a.keys + (size_t)(k_ok[i] ? kp : a.c0) * row4;
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
    if (!q_ok) return;
    // accumulator register j of tile i: key row (j & 3) + 8 (j >> 2) + 4 half, query column col -- four runs of four consecutive keys.
    // A tile that starts inside the chunk lies inside the row's C floats (C and the tile are multiples of 32): keys past the chunk's
    // end get the product of a zero operand there and are never read.
    bool bad = false;
    float *out = a.scores + (size_t)q * a.C;
#pragma unroll
    for (int i = 0; i < KT; ++i) {
        const int off = t_lo + i * CK;
        if (off >= a.len) continue;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int k0 = off + 8 * g + 4 * half;
            float4 v;                                              // (+ 0: theta = 0 times a negative product is -0; one zero, one tie)
            v.x = a.theta * acc[i][4 * g] + 0.0f;
            v.y = a.theta * acc[i][4 * g + 1] + 0.0f;
            v.z = a.theta * acc[i][4 * g + 2] + 0.0f;
            v.w = a.theta * acc[i][4 * g + 3] + 0.0f;
            bad |= (k0 < a.len && !isfinite(v.x)) | (k0 + 1 < a.len && !isfinite(v.y)) | (k0 + 2 < a.len && !isfinite(v.z)) |
                   (k0 + 3 < a.len && !isfinite(v.w));
            *(float4 *)(out + k0) = v;
        }
    }
    if (bad && a.flags) atomicOr(a.flags, 1);
}

// the order-preserving image of a float's bits: a < b (as floats, -0 below +0) <=> image(a) < image(b) (as unsigned)
__device__ inline unsigned image(float x) {
    const unsigned b = __float_as_uint(x);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ inline float unimage(unsigned u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u); }

// (score, index) as one integer: larger = earlier in the definition's order.  i < 2^24.
__device__ inline unsigned long long composite(float x, int i) { return ((unsigned long long)image(x) << 24) | (unsigned)(0xffffff - i); }

__global__ void __launch_bounds__(ST) memory_topk_select_kernel(const TopkArgs a) {
    __shared__ unsigned long long cand[2 * KMAX];
    __shared__ int hist[256], scan[2][256];
    __shared__ int sel_bin, sel_need, sel_all, n_cand;
    const int r = blockIdx.x, tid = threadIdx.x;
    if (r >= live_rows(a)) return;
    const float *sc = a.scores + (size_t)r * a.C;
    const int len = a.len;
    const int kk = min(a.K, len);                                  // winners of this chunk
    const int m_prev = min(a.K, a.c0);                             // entries of the running list

    // radix select: `prefix` holds the bytes fixed so far of the kk-th largest composite, `need` how many of the entries that agree
    // with it on those bytes are still wanted.  A pass ends the search when the whole bin is wanted: everything at or above the
    // prefix (lower bytes zero) is then taken.
    unsigned long long prefix = 0;
    int need = kk;
    for (int p = 0; p < 7; ++p) {
        const int shift = 8 * (6 - p);
        hist[tid] = 0;
        __syncthreads();
        for (int i0 = 4 * tid; i0 < len; i0 += 4 * ST) {
            const float4 v4 = *(const float4 *)(sc + i0);           // (inside the row's C floats: see the score kernel)
            const float v[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (i0 + e >= len) continue;
                const unsigned long long c = composite(v[e], a.c0 + i0 + e);
                if (p == 0 || (c >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[(int)(c >> shift) & 255], 1);
            }
        }
        __syncthreads();
        // above[t] = entries in the bins t + 1 .. 255: an inclusive suffix scan less the bin itself
        const int h = hist[tid];
        scan[0][tid] = h;
        __syncthreads();
        int cur = 0;
        for (int d = 1; d < 256; d <<= 1) {
            scan[cur ^ 1][tid] = scan[cur][tid] + (tid + d < 256 ? scan[cur][tid + d] : 0);
            cur ^= 1;
            __syncthreads();
        }
        const int above = scan[cur][tid] - h;
        if (above < need && need <= above + h) {                   // exactly one bin
            sel_bin = tid;
            sel_need = need - above;
            sel_all = (need - above == h);
        }
        __syncthreads();
        prefix |= (unsigned long long)sel_bin << shift;
        need = sel_need;
        const int all = sel_all;
        __syncthreads();
        if (all) break;
    }

    // gather the chunk's winners, append the running list, pad to a power of two with zeros (below every composite that matters)
    if (tid == 0) n_cand = 0;
    __syncthreads();
    for (int i0 = 4 * tid; i0 < len; i0 += 4 * ST) {
        const float4 v4 = *(const float4 *)(sc + i0);
        const float v[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (i0 + e >= len) continue;
            const unsigned long long c = composite(v[e], a.c0 + i0 + e);
            if (c >= prefix) {
                const int slot = atomicAdd(&n_cand, 1);
                if (slot < KMAX) cand[slot] = c;                   // (exactly kk <= K of them; the test keeps a wrong count in bounds)
            }
        }
    }
    unsigned long long *run = a.run + (size_t)r * a.K;
    for (int j = tid; j < m_prev; j += ST) cand[kk + j] = run[j];
    const int n2 = kk + m_prev;
    int P = 1;
    while (P < n2) P <<= 1;
    for (int j = n2 + tid; j < P; j += ST) cand[j] = 0;
    __syncthreads();

    // bitonic sort, descending
    for (int size = 2; size <= P; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < P / 2; t += ST) {
                const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
                const bool desc = (lo & size) == 0;
                const unsigned long long x = cand[lo], y = cand[hi];
                if ((x < y) == desc) {
                    cand[lo] = y;
                    cand[hi] = x;
                }
            }
            __syncthreads();
        }

    const int m = min(a.K, n2);
    if (!a.last) {
        for (int j = tid; j < m; j += ST) run[j] = cand[j];
        return;
    }
    for (int j = tid; j < m; j += ST) {
        const unsigned long long c = cand[j];
        const int i = 0xffffff - (int)(c & 0xffffff);
        if (i >= a.N) continue;                                    // (cannot happen: every composite of the list came from a key)
        a.s[(size_t)r * a.ld_s + j] = unimage((unsigned)(c >> 24));
        a.ret_words[(size_t)j * a.n_rows + r] = a.key_words[i];
        if (a.ret_idx) a.ret_idx[(size_t)j * a.n_rows + r] = i;
    }
}

inline long long round_up(long long x, long long m) { return (x + m - 1) / m * m; }

}  // namespace

// the smallest workspace: a chunk of one tile and the running lists (include/jlm_hip.h)
extern "C" size_t jlm_memory_topk_workspace_bytes(int N, int n_rows_max, int K) {
    if (N < 1 || N > JLM_MEMORY_MAX_KEYS || n_rows_max < 0 || K < 1 || K > JLM_MEMORY_TOPK_MAX) return 0;
    return (size_t)n_rows_max * ((size_t)CK * sizeof(float) + (size_t)K * sizeof(unsigned long long));
}

// keys per chunk at a workspace of `workspace_bytes`: a multiple of 32, at most N rounded up to one; 0 where the launcher refuses
extern "C" int jlm_memory_topk_chunk_keys(int N, int n_rows_max, int K, size_t workspace_bytes) {
    const size_t need = jlm_memory_topk_workspace_bytes(N, n_rows_max, K);
    if (need == 0 && n_rows_max != 0) return 0;
    if (N < 1 || N > JLM_MEMORY_MAX_KEYS || n_rows_max < 0 || K < 1 || K > JLM_MEMORY_TOPK_MAX || workspace_bytes < need) return 0;
    const long long whole = round_up(N, CK);
    if (n_rows_max == 0) return (int)whole;
    const size_t lists = (size_t)n_rows_max * K * sizeof(unsigned long long);
    const size_t c = (workspace_bytes - lists) / ((size_t)n_rows_max * sizeof(float)) / CK * CK;
    return (int)(c < (size_t)whole ? c : (size_t)whole);
}

// the launcher's refusals on their own (jlm_rank_memory_frames asks before its first launch): -1, or 0
int jlm_memory_topk_refuse(const void *keys, const int *key_words, int N, int H, int split, float h_scale, const void *q_rows, int n_rows_max,
                           const int *n_dev, float theta, int K, const float *s, int ld_s, const int *ret_words, const int *ret_idx, int n_rows,
                           const void *workspace, size_t workspace_bytes, const int *flags) {
    if (N < 1 || N > JLM_MEMORY_MAX_KEYS || K < 1 || K > JLM_MEMORY_TOPK_MAX || ld_s < K) return -1;
    if (H <= 0 || H % 32 != 0) return -1;                          // what jlm_lstm_step / jlm_lstm_step_xg accept
    if (!(theta >= 0.0f) || !isfinite(theta)) return -1;
    if (split && !(h_scale > 0.0f && isfinite(h_scale))) return -1;
    if (n_rows < 0 || n_rows > 65535 || n_rows_max < 0 || n_rows_max > n_rows) return -1;
    if (n_rows_max == 0) return 0;
    if (!keys || !key_words || !q_rows || !s || !ret_words || !workspace) return -1;
    if ((((uintptr_t)keys | (uintptr_t)q_rows | (uintptr_t)workspace) & 15) != 0) return -1;
    if ((((uintptr_t)key_words | (uintptr_t)n_dev | (uintptr_t)s | (uintptr_t)ret_words | (uintptr_t)ret_idx | (uintptr_t)flags) & 3) != 0) return -1;
    if (workspace_bytes < jlm_memory_topk_workspace_bytes(N, n_rows_max, K)) return -1;
    return 0;
}

extern "C" int jlm_memory_topk(const void *keys, const int *key_words, int N, int H, int split, float h_scale, const void *q_rows,
                               int n_rows_max, const int *n_dev, float theta, int K, float *s, int ld_s, int *ret_words, int *ret_idx,
                               int n_rows, void *workspace, size_t workspace_bytes, int *flags, void *stream) {
    if (int rc = jlm_memory_topk_refuse(keys, key_words, N, H, split, h_scale, q_rows, n_rows_max, n_dev, theta, K, s, ld_s, ret_words, ret_idx,
                                        n_rows, workspace, workspace_bytes, flags))
        return rc;
    if (n_rows_max == 0) return 0;
    TopkArgs a;
    a.keys = (const uint4 *)keys; a.q_rows = (const uint4 *)q_rows; a.key_words = key_words; a.n_dev = n_dev;
    a.C = jlm_memory_topk_chunk_keys(N, n_rows_max, K, workspace_bytes);
    a.scores = (float *)workspace;
    a.run = (unsigned long long *)((char *)workspace + (size_t)n_rows_max * a.C * sizeof(float));   // (C % 32 == 0: 8-byte aligned)
    a.s = s; a.ret_words = ret_words; a.ret_idx = ret_idx; a.flags = flags;
    a.N = N; a.H = H; a.K = K; a.n_rows_max = n_rows_max; a.n_rows = n_rows; a.ld_s = ld_s;
    a.theta = split ? theta / (h_scale * h_scale) : theta;
    for (int c0 = 0; c0 < N; c0 += a.C) {
        a.c0 = c0; a.len = N - c0 < a.C ? N - c0 : a.C; a.last = c0 + a.len == N;
        const dim3 grid((n_rows_max + CQ - 1) / CQ, (a.len + WG_KEYS - 1) / WG_KEYS);   // query block fastest: co-resident workgroups share keys
        if (split)
            memory_topk_score_kernel<true><<<grid, dim3(CW * 64), 0, (hipStream_t)stream>>>(a);
        else
            memory_topk_score_kernel<false><<<grid, dim3(CW * 64), 0, (hipStream_t)stream>>>(a);
        if (int rc = (int)hipGetLastError()) return rc;
        memory_topk_select_kernel<<<dim3(n_rows_max), dim3(ST), 0, (hipStream_t)stream>>>(a);
        if (int rc = (int)hipGetLastError()) return rc;
    }
    return 0;
}
