// jlm_memory.hip -- scoring against a memory of hidden states (include/jlm_hip.h jlm_memory_rows): one store of
// (k_i, v_i) pairs, shared by every query of every call, where section 18's cache is a window of the query's own row.
//
// memory_rows_kernel keeps cache_rows_kernel's lane layout (csrc/jlm_cache.hip) -- keys are the MFMA rows, queries the MFMA columns, a
// lane owns one query and sixteen keys of a 32-key tile, its Online {m, Z, M} per theta stays in registers and nothing crosses lanes
// inside the key loop -- with two differences.  Queries and keys come from different arrays: no ring, no wrap, no causal mask, every
// query sees every key.  And the grid is (block of 32 queries) x (key split): a workgroup reads the keys [split * S, split * S + S) of
// the memory, S = jlm_memory_keys_per_split(N), wave w taking the tile pairs w, w + 8, ... of that range, folds its sixteen partial
// states of a query in cache_rows_kernel's fixed order and writes ONE partial (m, Z, M) per (theta, split, query) to the workspace.
// memory_fold_kernel folds a query's splits in ascending order and writes logf(M) - logf(Z).
//
// What a query's bits depend on: its own state row and word, the memory, theta.  The column a query sits in, the other queries of its
// block, the number of thetas and the workspace's earlier content do not enter: an MFMA column is a function of its own B operand and
// the A rows, a lane updates no state but its own, every partial a fold reads was written by this launch, and S depends on N alone.
// The grid's x dimension is the query block, so workgroups that run at the same time share a key split (blocks go round-robin over the
// chip's L2 domains in x-fastest order): a key tile is expected in an L2 once per resident wave of query blocks.  Not measured.
// Plain vector loads and stores, one writer per address; the only atomic is the OR on the flag word.
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

struct MemoryArgs {
    const uint4 *keys, *q_rows;
    const int *key_words, *q_words, *len;
    float *ws;                                  // [n_theta][n_split][3][n_query]
    int *flags;
    int N, H, S, n_split, n_rows, n_query, n_theta;
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
__global__ void __launch_bounds__(CW * 64) memory_rows_kernel(const MemoryArgs a) {
    __shared__ float red[JLM_CACHE_MAX_THETAS][CW][3][CQ];
    const int q_lo = blockIdx.x * CQ, sp = blockIdx.y;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int col = lane & 31, half = lane >> 5;
    const int k_lo = sp * a.S;                                     // this workgroup's keys: k_lo <= i < k_hi
    const int k_hi = min(k_lo + a.S, a.N);
    const int n_keys = k_hi - k_lo;
    const size_t row4 = (size_t)a.H / 4;                           // 16-byte records of a state row

    // this lane's query: column `col`, query q = t * n_rows + r, live iff t < len[r]
    const int q = q_lo + col;
    bool q_ok = q < a.n_query;
    if (q_ok && a.len) q_ok = q / a.n_rows < a.len[q % a.n_rows];
    if (__ballot(q_ok) == 0) return;                               // (every wave holds all 32 columns, so this is uniform over the
                                                                   //  workgroup: a block without a live query writes nothing)
    const uint4 *q_row = a.q_rows + (size_t)(q_ok ? q : 0) * row4;
    const int q_word = q_ok ? a.q_words[q] : 0;

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
            k_row[i] = a.keys + (size_t)(k_ok[i] ? kp : k_lo) * row4;
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
                if (q_ok && kp < k_hi) {
                    ok |= 1u << j;
                    if (a.key_words[kp] == q_word) match |= 1u << j;
                    if (!isfinite(acc[i][j])) bad = true;
                }
            }
#pragma unroll
            for (int t = 0; t < JLM_CACHE_MAX_THETAS; ++t) {
                if (!ok || t >= a.n_theta) continue;               // (no break: the loop must unroll, st[] stays in registers)
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
    // the workgroup's partial of query q_lo + n: written by the thread whose own column n is -- it knows whether the query is live
    for (int t = w; t < a.n_theta; t += CW) {
        if (half != 0 || !q_ok) continue;
        float mx = -INFINITY;
        for (int i = 0; i < CW; ++i) mx = fmaxf(mx, red[t][i][0][col]);
        float Z = 0.0f, M = 0.0f;
        if (mx > -INFINITY)
            for (int i = 0; i < CW; ++i) {
                const float e = expf(red[t][i][0][col] - mx);       // (a wave without a key: exp(-inf) = 0)
                Z += red[t][i][1][col] * e;
                M += red[t][i][2][col] * e;
            }
        float *p = a.ws + ((size_t)t * a.n_split + sp) * 3 * (size_t)a.n_query + q;
        p[0] = mx;
        p[(size_t)a.n_query] = Z;
        p[2 * (size_t)a.n_query] = M;
    }
}

// one thread per (theta, query): the splits' partials in ascending order -> lpm
__global__ void __launch_bounds__(256) memory_fold_kernel(const float *__restrict__ ws, const int *__restrict__ len, float *__restrict__ lpm,
                                                          int n_rows, int n_query, int n_split, int n_theta) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)n_theta * n_query) return;
    const int t = (int)(idx / n_query), q = (int)(idx % n_query);
    if (len && q / n_rows >= len[q % n_rows]) return;               // entries of rows that are not live are left untouched
    const float *p = ws + (size_t)t * n_split * 3 * (size_t)n_query + q;
    const size_t nq = (size_t)n_query;
    float mx = -INFINITY;
    for (int i = 0; i < n_split; ++i) mx = fmaxf(mx, p[(size_t)i * 3 * nq]);
    float out = -INFINITY;
    if (mx > -INFINITY) {
        float Z = 0.0f, M = 0.0f;
        for (int i = 0; i < n_split; ++i) {
            const float e = expf(p[(size_t)i * 3 * nq] - mx);
            Z += p[(size_t)i * 3 * nq + nq] * e;
            M += p[(size_t)i * 3 * nq + 2 * nq] * e;
        }
        out = logf(M) - logf(Z);                                    // (no match: log 0 = -inf exactly)
    }
    lpm[idx] = out;
}

}  // namespace

// keys per split: a function of N alone (include/jlm_hip.h)
extern "C" int jlm_memory_keys_per_split(int N) {
    if (N < 1 || N > JLM_MEMORY_MAX_KEYS) return 0;
    const long long per = ((long long)N + JLM_MEMORY_MAX_SPLITS - 1) / JLM_MEMORY_MAX_SPLITS;
    const long long s = (per + 63) / 64 * 64;
    return (int)(s < JLM_MEMORY_MIN_SPLIT_KEYS ? JLM_MEMORY_MIN_SPLIT_KEYS : s);
}

static int memory_splits(int N) {
    const int S = jlm_memory_keys_per_split(N);
    return (N + S - 1) / S;
}

extern "C" size_t jlm_memory_workspace_bytes(int N, int n_rows, int n_steps, int n_theta) {
    if (N < 1 || N > JLM_MEMORY_MAX_KEYS || n_rows < 0 || n_steps < 0 || n_theta < 1) return 0;
    return (size_t)n_theta * memory_splits(N) * 3 * (size_t)n_rows * n_steps * sizeof(float);
}

// the launcher's refusals on their own (jlm_score_memory_frames asks before its first launch): -1, or 0
int jlm_memory_refuse(const void *keys, const int *key_words, int N, int H, int split, float h_scale, const void *q_rows, const int *q_words,
                      int n_rows, int n_steps, const int *len, const float *thetas, int n_theta, const float *lpm, const void *workspace,
                      size_t workspace_bytes, const int *flags) {
    if (n_rows < 0 || n_steps < 0 || N < 1 || N > JLM_MEMORY_MAX_KEYS) return -1;
    if (H <= 0 || H % 32 != 0) return -1;                          // what jlm_lstm_step / jlm_lstm_step_xg accept
    if (n_theta < 1 || n_theta > JLM_CACHE_MAX_THETAS || !thetas) return -1;
    for (int t = 0; t < n_theta; ++t)
        if (!(thetas[t] >= 0.0f) || !isfinite(thetas[t])) return -1;
    if (split && !(h_scale > 0.0f && isfinite(h_scale))) return -1;
    if (n_rows == 0 || n_steps == 0) return 0;
    if (n_rows > 65535 || (long long)n_rows * n_steps > 0x7fffff00ll / JLM_CACHE_MAX_THETAS) return -1;
    if (!keys || !key_words || !q_rows || !q_words || !lpm || !workspace) return -1;
    if ((((uintptr_t)keys | (uintptr_t)q_rows) & 15) != 0) return -1;
    if ((((uintptr_t)key_words | (uintptr_t)q_words | (uintptr_t)len | (uintptr_t)lpm | (uintptr_t)workspace | (uintptr_t)flags) & 3) != 0) return -1;
    if (workspace_bytes < jlm_memory_workspace_bytes(N, n_rows, n_steps, n_theta)) return -1;
    return 0;
}

extern "C" int jlm_memory_rows(const void *keys, const int *key_words, int N, int H, int split, float h_scale, const void *q_rows,
                               const int *q_words, int n_rows, int n_steps, const int *len, const float *thetas, int n_theta, float *lpm,
                               void *workspace, size_t workspace_bytes, int *flags, void *stream) {
    if (int rc = jlm_memory_refuse(keys, key_words, N, H, split, h_scale, q_rows, q_words, n_rows, n_steps, len, thetas, n_theta, lpm, workspace,
                                   workspace_bytes, flags))
        return rc;
    if (n_rows == 0 || n_steps == 0) return 0;
    MemoryArgs a;
    a.keys = (const uint4 *)keys; a.q_rows = (const uint4 *)q_rows; a.key_words = key_words; a.q_words = q_words; a.len = len;
    a.ws = (float *)workspace; a.flags = flags;
    a.N = N; a.H = H; a.S = jlm_memory_keys_per_split(N); a.n_split = memory_splits(N);
    a.n_rows = n_rows; a.n_query = n_rows * n_steps; a.n_theta = n_theta;
    for (int t = 0; t < JLM_CACHE_MAX_THETAS; ++t)
        a.theta[t] = t < n_theta ? (split ? thetas[t] / (h_scale * h_scale) : thetas[t]) : 0.0f;
    const dim3 grid((a.n_query + CQ - 1) / CQ, a.n_split);           // query block fastest: co-resident workgroups share a key split
    if (split)
        memory_rows_kernel<true><<<grid, dim3(CW * 64), 0, (hipStream_t)stream>>>(a);
    else
        memory_rows_kernel<false><<<grid, dim3(CW * 64), 0, (hipStream_t)stream>>>(a);
    if (int rc = (int)hipGetLastError()) return rc;
    const size_t n_out = (size_t)n_theta * a.n_query;
    memory_fold_kernel<<<dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, (hipStream_t)stream>>>(a.ws, len, lpm, n_rows, a.n_query, a.n_split,
                                                                                                     n_theta);
    return (int)hipGetLastError();
}
