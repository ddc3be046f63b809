// jlm_cache_mix.hip -- the continuous cache on the decode side (include/jlm_hip.h jlm_cache_query / jlm_cache_mix_rows; DESIGN.md
// section 20): the cache distribution over EVERY word of a row's window, as a patch of the row's materialised logits, so that
// rank_rows_kernel and topk_rows_kernel run unchanged on the mixed distribution.
//
// cache_query_kernel -- s[r][j] = theta' (h_q . h_i) of ONE query a row (the state row a step just wrote) against the row's window in
// the rings of jlm_cache_rows.  Grid (chunk of CQ_KEYS keys, row); four lanes a key, lane `sub` of the four owning the 32-byte units
// sub, sub + 4, ... of the key row (a unit = eight values: two 16-byte records, on split rows [8 hi][8 lo]), an f32 fmaf chain over
// its units in k order, then (a0 + a1) + (a2 + a3) through two lane exchanges.  The partition and the fold are fixed by H alone, so the
// bits of s[r][j] are a function of the two rows and theta: not of pos, cap, the chunk or the launch's row count.  The pass is a
// stream over rows * n_q * H * 4 bytes; the VALU keeps up with it, and the matrix pipe would tie the order of the sum to the tile.
//
// cache_mix_rows_kernel -- one workgroup of 256 threads per live row.  The row's s and the window's words go to LDS (12 N bytes with
// e_j); the maximum, e_j = expf(s_j - max) and Z are formed in a fixed tree over j (thread t owns j = t, t + 256, ... in ascending
// order, an xor tree over the wave, the four waves in order); c(w) is summed over the entries with w_j = w in ascending j by the thread
// that owns the FIRST occurrence of w, so a word has one writer and nothing is atomic -- every lane of a wave reads the same word of
// the LDS array in the all-pairs loop (a broadcast: no bank conflict).  L is the row's log-normaliser by rl_row (csrc/jlm_row_lse.h),
// the function topk_rows_kernel's is built from, read before any word is patched.  y[w] <- logaddexp(y[w], L + log rho + log c - log Z).
#include <math.h>
#include "jlm_common.h"
#include "jlm_cache_unit.h"
#include "jlm_row_lse.h"

namespace {

constexpr int CQ_KEYS = 64;            // keys per workgroup of cache_query_kernel: 256 threads, four lanes a key
constexpr int CM_THREADS = 256;
constexpr int CM_WAVES = CM_THREADS / 64;
constexpr int CM_JPT = JLM_CACHE_MIX_MAX_N / CM_THREADS;          // window entries a thread owns at most

static_assert(CM_JPT * CM_THREADS == JLM_CACHE_MIX_MAX_N && CM_JPT == 16, "cm_pairs_patch is instantiated for 1, 2, 4, 8 and 16 entries");

static_assert(CM_WAVES == RL_WAVES, "rl_row (csrc/jlm_row_lse.h) is called by a workgroup of RL_WAVES waves");

struct QueryArgs {
    const uint4 *hist, *q;
    const int *first, *n_dev;
    float *s;
    int *flags;
    int cap, n_rows, n_rows_max, H, pos, N, ld_s;
    float theta;                       // split rows: theta / h_scale^2
};

// (Rec and cq_unit, the decode of one 32-byte unit of a state row: csrc/jlm_cache_unit.h, shared with cache_cell_query_kernel)
template <bool SPLIT>
__global__ void __launch_bounds__(4 * CQ_KEYS) cache_query_kernel(const QueryArgs a) {
    const int r = blockIdx.y;
    const int live = min(a.n_dev ? *a.n_dev : a.n_rows_max, a.n_rows_max);
    if (r >= live) return;
    const int lo = max(max(a.pos - a.N, a.first[r]), 0);
    const int n_q = a.pos - lo;
    if ((int)blockIdx.x * CQ_KEYS >= n_q) return;                  // (block-uniform; an empty window writes nothing)
    const int j = blockIdx.x * CQ_KEYS + (threadIdx.x >> 2), sub = threadIdx.x & 3;
    const bool ok = j < n_q;                                       // (the four lanes of a key agree)
    const size_t row4 = (size_t)a.H / 4;
    const uint4 *k_row = a.hist + ((size_t)((lo + (ok ? j : 0)) % a.cap) * a.n_rows + r) * row4;
    const uint4 *q_row = a.q + (size_t)r * row4;
    float acc = 0.0f;
    if (ok) {
#pragma unroll 2
        for (int u = sub; u < a.H / 8; u += 4) {
            float kv[8], qv[8];
            cq_unit<SPLIT>(k_row, u, kv);
            cq_unit<SPLIT>(q_row, u, qv);
#pragma unroll
            for (int i = 0; i < 8; ++i) acc = fmaf(qv[i], kv[i], acc);
        }
    }
    acc = acc + __shfl_xor(acc, 1);                                // a0 + a1 | a2 + a3 (the same bits on both lanes of a pair)
    acc = acc + __shfl_xor(acc, 2);
    const float sv = a.theta * acc;
    if (ok && sub == 0) {
        a.s[(size_t)r * a.ld_s + j] = sv;
        if (!isfinite(sv) && a.flags) atomicOr(a.flags, 1);
    }
}

struct MixArgs {
    float *y;
    const float *s;
    const int *words, *first, *n_dev;
    float *lpc_ent;
    int *flags;
    int ld_y, n_cols, ld_s, cap, n_rows, n_rows_max, pos, N;
    float log_rho;                     // log(lambda / (1 - lambda))
};

// The all-pairs pass and the patch.  A thread owns the entries j = tid + 256 u, u < JPT, in registers; the window is walked ONCE, four
// entries i a trip (two 16-byte LDS reads at one address a wave: broadcasts), and every owned j takes from entry i what is its: a
// repeat mark when w_i = w_j and i < j, e_i into c when w_i = w_j and i >= j.  Each c is still the sum over its matches in ascending
// i (+ 0 is exact), whatever JPT is; the padding of the last trip holds e = 0 and the word -1.
template <int JPT>
__device__ __forceinline__ void cm_pairs_patch(const MixArgs &a, int r, int n_q, const int *sh_w, const float *sh_e, float *yrow, float base,
                                               float log_z) {
    const int tid = threadIdx.x;
    int wj[JPT];
    float cj[JPT];
    unsigned rep = 0;
#pragma unroll
    for (int u = 0; u < JPT; ++u) {
        const int j = tid + u * CM_THREADS;
        wj[u] = j < n_q ? sh_w[j] : 0;                             // (an entry the thread does not have: its results are dropped below)
        cj[u] = 0.0f;
    }
    for (int i0 = 0; i0 < n_q; i0 += 4) {
        const int4 w4 = *reinterpret_cast<const int4 *>(sh_w + i0);
        const float4 e4 = *reinterpret_cast<const float4 *>(sh_e + i0);
        const int wi[4] = {w4.x, w4.y, w4.z, w4.w};
        const float ei[4] = {e4.x, e4.y, e4.z, e4.w};
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int u = 0; u < JPT; ++u) {
                const bool same = wi[k] == wj[u], before = i0 + k < tid + u * CM_THREADS;
                rep |= (same && before ? 1u : 0u) << u;
                cj[u] += same && !before ? ei[k] : 0.0f;
            }
    }
#pragma unroll
    for (int u = 0; u < JPT; ++u) {
        const int j = tid + u * CM_THREADS, w = wj[u];
        if (j >= n_q) continue;
        const bool repeat = (rep >> u) & 1u;
        const float lpc = repeat ? -INFINITY : logf(cj[u]) - log_z;
        if (a.lpc_ent) a.lpc_ent[(size_t)r * a.ld_s + j] = lpc;
        if (repeat || w < 0 || w >= a.n_cols) continue;
        const float yw = yrow[w], t = base + lpc;
        if (t > -INFINITY && yw == yw) yrow[w] = jlm_logaddexpf(yw, t);
    }
}

template <int SELF_NORM>
__global__ void __launch_bounds__(CM_THREADS) cache_mix_rows_kernel(const MixArgs a) {
    extern __shared__ uint4 cm_lds[];                              // [Np] s, [Np] words, [Np] e; Np = N rounded up to 4
    __shared__ float r_max[CM_WAVES], r_z[CM_WAVES], l_m[CM_WAVES];
    __shared__ double l_s[CM_WAVES];
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int live = min(a.n_dev ? *a.n_dev : a.n_rows_max, a.n_rows_max);
    if (r >= live) return;
    const int lo = max(max(a.pos - a.N, a.first[r]), 0);
    const int n_q = a.pos - lo;
    if (n_q <= 0) return;                                          // an empty window: the row's bits stay
    const int n_pad = (a.N + 3) & ~3;                              // (16-byte reads of the word and e arrays)
    float *sh_s = reinterpret_cast<float *>(cm_lds);
    int *sh_w = reinterpret_cast<int *>(sh_s + n_pad);
    float *sh_e = reinterpret_cast<float *>(sh_w + n_pad);

    float mx = -INFINITY;
    int bad = 0, oor = 0;
    for (int j = tid; j < n_q; j += CM_THREADS) {
        const float sj = a.s[(size_t)r * a.ld_s + j];
        const int wj = a.words[(size_t)((lo + j) % a.cap) * a.n_rows + r];
        sh_s[j] = sj;
        sh_w[j] = wj;
        mx = fmaxf(mx, sj);
        bad |= !isfinite(sj);
        oor |= wj < 0 || wj >= a.n_cols;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
    if (lane == 0) r_max[wv] = mx;
    bad = __syncthreads_or(bad);
    oor = __syncthreads_or(oor);
    if (tid == 0 && a.flags && (bad || oor)) atomicOr(a.flags, (bad ? 1 : 0) | (oor ? 4 : 0));
    if (bad) return;                                               // a score that is not finite: the row is left as it is
    mx = fmaxf(fmaxf(r_max[0], r_max[1]), fmaxf(r_max[2], r_max[3]));

    float z = 0.0f;
    for (int j = tid; j < n_q; j += CM_THREADS) {
        const float e = expf(sh_s[j] - mx);
        sh_e[j] = e;
        z += e;
    }
    if (tid < ((n_q + 3) & ~3) - n_q) {                            // the padding of the all-pairs pass' last trip
        sh_w[n_q + tid] = -1;
        sh_e[n_q + tid] = 0.0f;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) z = z + __shfl_xor(z, off);
    if (lane == 0) r_z[wv] = z;

    float *yrow = a.y + (size_t)r * a.ld_y;
    float L = 0.0f;
    if (!SELF_NORM) {
        float M;
        double S;
        rl_row(reinterpret_cast<const f32x4 *>(yrow), a.n_cols, l_m, l_s, M, S);
        if (!(M > -INFINITY && M < INFINITY && S > 0.0 && S < INFINITY)) {                   // (block-uniform)
            if (tid == 0 && a.flags) atomicOr(a.flags, 2);
            return;
        }
        L = (float)((double)M + log(S));
    } else {
        __syncthreads();
    }
    const float Z = ((r_z[0] + r_z[1]) + r_z[2]) + r_z[3];
    const float log_z = logf(Z);
    const float base = L + a.log_rho;

    const int n_u = (n_q + CM_THREADS - 1) / CM_THREADS;           // entries a thread owns (block-uniform)
    if (n_u <= 1) cm_pairs_patch<1>(a, r, n_q, sh_w, sh_e, yrow, base, log_z);
    else if (n_u <= 2) cm_pairs_patch<2>(a, r, n_q, sh_w, sh_e, yrow, base, log_z);
    else if (n_u <= 4) cm_pairs_patch<4>(a, r, n_q, sh_w, sh_e, yrow, base, log_z);
    else if (n_u <= 8) cm_pairs_patch<8>(a, r, n_q, sh_w, sh_e, yrow, base, log_z);
    else cm_pairs_patch<CM_JPT>(a, r, n_q, sh_w, sh_e, yrow, base, log_z);
}

// what both launchers refuse of the rings and the window: -1, or 0
int cm_refuse_rings(int cap, int n_rows, int n_rows_max, int pos, const int *first, const int *n_dev, int N, int ld_s, const int *flags) {
    if (n_rows < 0 || n_rows_max < 0 || n_rows_max > n_rows || N < 1 || N > JLM_CACHE_MIX_MAX_N || cap < N || pos < 0 || ld_s < N) return -1;
    if ((long long)pos + cap > 0x7fffffffll) return -1;
    if (n_rows_max == 0) return 0;
    if (n_rows_max > 65535 || !first) return -1;
    if ((((uintptr_t)first | (uintptr_t)n_dev | (uintptr_t)flags) & 3) != 0) return -1;
    return 0;
}

}  // namespace

// the refusals of jlm_cache_query on their own (jlm_rank_cache_frames and jlm_predict_cache_rows ask before their first launch, with
// the last position of the call): -1, or 0
int jlm_cache_query_refuse(const void *hist, int cap, int n_rows, int H, int split, float h_scale, const void *q_rows, int n_rows_max,
                           const int *n_dev, int pos, const int *first, int N, float theta, const float *s, int ld_s, const int *flags) {
    if (int rc = cm_refuse_rings(cap, n_rows, n_rows_max, pos, first, n_dev, N, ld_s, flags)) return rc;
    if (H <= 0 || H % 32 != 0) return -1;                          // what jlm_lstm_step / jlm_lstm_step_xg accept
    if (!(theta >= 0.0f) || !isfinite(theta)) return -1;
    if (split && !(h_scale > 0.0f && isfinite(h_scale))) return -1;
    if (n_rows_max == 0) return 0;
    if (!hist || !q_rows || !s) return -1;
    if ((((uintptr_t)hist | (uintptr_t)q_rows) & 15) != 0 || ((uintptr_t)s & 3) != 0) return -1;
    return 0;
}

// the refusals of jlm_cache_mix_rows on their own
int jlm_cache_mix_refuse(const float *y, int ld_y, int n_cols, const float *s, int ld_s, const int *words, int cap, int n_rows,
                         int n_rows_max, const int *n_dev, int pos, const int *first, int N, float lam, const float *lpc_ent,
                         const int *flags) {
    if (int rc = cm_refuse_rings(cap, n_rows, n_rows_max, pos, first, n_dev, N, ld_s, flags)) return rc;
    if (!(lam >= 0.0f && lam < 1.0f)) return -1;
    if (n_cols < 1 || ld_y % 4 != 0 || ld_y < ((n_cols + 3) & ~3)) return -1;
    if (n_rows_max == 0) return 0;
    if (!y || !s || !words || ((uintptr_t)y & 15) != 0 || (((uintptr_t)s | (uintptr_t)words | (uintptr_t)lpc_ent) & 3) != 0) return -1;
    return 0;
}

extern "C" int jlm_cache_query(const void *hist, int cap, int n_rows, int H, int split, float h_scale, const void *q_rows, int n_rows_max,
                               const int *n_dev, int pos, const int *first, int N, float theta, float *s, int ld_s, int *flags,
                               void *stream) {
    if (int rc = jlm_cache_query_refuse(hist, cap, n_rows, H, split, h_scale, q_rows, n_rows_max, n_dev, pos, first, N, theta, s, ld_s, flags))
        return rc;
    if (n_rows_max == 0) return 0;
    QueryArgs a;
    a.hist = (const uint4 *)hist; a.q = (const uint4 *)q_rows; a.first = first; a.n_dev = n_dev; a.s = s; a.flags = flags;
    a.cap = cap; a.n_rows = n_rows; a.n_rows_max = n_rows_max; a.H = H; a.pos = pos; a.N = N; a.ld_s = ld_s;
    a.theta = split ? theta / (h_scale * h_scale) : theta;
    const dim3 grid((N + CQ_KEYS - 1) / CQ_KEYS, n_rows_max);
    if (split)
        cache_query_kernel<true><<<grid, dim3(4 * CQ_KEYS), 0, (hipStream_t)stream>>>(a);
    else
        cache_query_kernel<false><<<grid, dim3(4 * CQ_KEYS), 0, (hipStream_t)stream>>>(a);
    return (int)hipGetLastError();
}

extern "C" int jlm_cache_mix_rows(float *y, int ld_y, int n_cols, int self_norm, const float *s, int ld_s, const int *words, int cap,
                                  int n_rows, int n_rows_max, const int *n_dev, int pos, const int *first, int N, float lam,
                                  float *lpc_ent, int *flags, void *stream) {
    if (int rc = jlm_cache_mix_refuse(y, ld_y, n_cols, s, ld_s, words, cap, n_rows, n_rows_max, n_dev, pos, first, N, lam, lpc_ent, flags))
        return rc;
    if (n_rows_max == 0) return 0;
    if (lam == 0.0f) return 0;                                     // p_q = p_lm: nothing to launch
    MixArgs a;
    a.y = y; a.s = s; a.words = words; a.first = first; a.n_dev = n_dev; a.lpc_ent = lpc_ent; a.flags = flags;
    a.ld_y = ld_y; a.n_cols = n_cols; a.ld_s = ld_s; a.cap = cap; a.n_rows = n_rows; a.n_rows_max = n_rows_max; a.pos = pos; a.N = N;
    a.log_rho = (float)(log((double)lam) - log1p(-(double)lam));
    const size_t lds = (size_t)12 * ((N + 3) & ~3);
    if (self_norm)
        cache_mix_rows_kernel<1><<<dim3(n_rows_max), dim3(CM_THREADS), lds, (hipStream_t)stream>>>(a);
    else
        cache_mix_rows_kernel<0><<<dim3(n_rows_max), dim3(CM_THREADS), lds, (hipStream_t)stream>>>(a);
    return (int)hipGetLastError();
}
