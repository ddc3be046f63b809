// jlm_cache_edge.hip -- the continuous cache inside the decode's frame loop (include/jlm_hip.h jlm_cache_cell_query /
// jlm_cache_cell_patch): the cache mass of every lattice edge leaving a frame, as a rewrite of the edge-logit
// buffer the next beam step reads.  The window of a sentence is fixed for the whole decode (the states and words of its left context,
// a CachedContext), so the hypotheses of a cell share their keys.
//
// cache_cell_query_kernel -- grid (chunk of CE_KEYS keys, sentence).  The workgroup stages the cell's query rows in LDS, CE_QG at a
// time, and dots every key of its chunk against each of them: a key comes from HBM once per cell (the passes over further groups of
// slots find it in L2), where one query a workgroup (cache_query_kernel) would read it once per hypothesis.  Per (query, key): four
// lanes a key, lane `sub` owning the 32-byte units sub, sub + 4, ..., an f32 fmaf chain in k order, (a0 + a1) + (a2 + a3) -- the
// partition, the order and the operand decode of cache_query_kernel (csrc/jlm_cache_unit.h), so s is bit-equal to jlm_cache_query's.
//
// cache_cell_patch_kernel -- one workgroup of 256 threads per sentence.  Wave 0 folds the cell's normaliser slices into lse with the
// beam step's own fold (csrc/jlm_beam_fold.h); the window's words go to LDS; wave w takes the slots w, w + 4, ...: the maximum, e_i
// (written back over s) and Z in a fixed tree (lane l owns i = l, l + 64, ... ascending, an xor tree); then thread p takes the
// positions p, p + 256, ... of the cell's word list: the window is walked once per group of CE_QG slots, four words a trip (one
// 16-byte LDS read at one address a wave: a broadcast), M summed in ascending i, and every edge logit of the position rewritten in
// f64.  The match structure is the same for every slot of a cell: a position without a match in the first group's walk walks no more.
#include <math.h>
#include "jlm_common.h"
#include "jlm_beam_fold.h"
#include "jlm_cache_unit.h"

namespace {

constexpr int CE_KEYS = 64;            // keys per workgroup of cache_cell_query_kernel: 256 threads, four lanes a key (CQ_KEYS)
constexpr int CE_QG = 8;               // query rows (slots) a pass: their accumulators stay in registers whatever the beam
constexpr int CE_THREADS = 256;
constexpr int CE_WAVES = CE_THREADS / 64;

struct CellQueryArgs {
    const uint4 *h, *hist;
    const int *g0, *cnt, *sent_len, *count, *idx;
    float *s;
    int *flags;
    int H, frame, beam, cap, n_src, N, ld_s;
    float theta;                       // split rows: theta / h_scale^2
};

// the window of sentence j: its cache row and entry count (0: none)
__device__ __forceinline__ int ce_window(const int *idx, const int *count, int j, int n_src, int cap, int N, int &r) {
    r = idx[j];
    if (r < 0 || r >= n_src) return 0;
    return max(min(min(count[r], cap), N), 0);
}

template <bool SPLIT>
__global__ void __launch_bounds__(4 * CE_KEYS) cache_cell_query_kernel(const CellQueryArgs a) {
    extern __shared__ uint4 ce_q[];                                // [CE_QG][H / 4]: the group's query rows as they are in the pool
    const int j = blockIdx.y, tid = threadIdx.x;
    if (a.frame >= a.sent_len[j]) return;                          // (everything up to the loop is block-uniform)
    int r;
    const int n = ce_window(a.idx, a.count, j, a.n_src, a.cap, a.N, r);
    const int kcnt = min(a.cnt[j], a.beam);
    if ((int)blockIdx.x * CE_KEYS >= n || kcnt <= 0) return;
    const int i = blockIdx.x * CE_KEYS + (tid >> 2), sub = tid & 3;
    const bool ok = i < n;                                         // (the four lanes of a key agree)
    const int row4 = a.H / 4;
    const uint4 *k_row = a.hist + ((size_t)(a.cap - n + (ok ? i : 0)) * a.n_src + r) * row4;
    const uint4 *q_rows = a.h + (size_t)a.g0[j] * row4;
    float *s_out = a.s + (size_t)j * a.beam * a.ld_s + i;
    for (int k0 = 0; k0 < kcnt; k0 += CE_QG) {
        const int ng = min(CE_QG, kcnt - k0);
        if (k0) __syncthreads();                                   // the previous group's rows have been read
        for (int t = tid; t < CE_QG * row4; t += 4 * CE_KEYS) {
            const int q = t / row4, c = t - q * row4;              // (a slot past the group: its last row again, the result dropped)
            ce_q[t] = q_rows[(size_t)(k0 + min(q, ng - 1)) * row4 + c];
        }
        __syncthreads();
        float acc[CE_QG];
#pragma unroll
        for (int q = 0; q < CE_QG; ++q) acc[q] = 0.0f;
        if (ok) {
            for (int u = sub; u < a.H / 8; u += 4) {
                float kv[8];
                cq_unit<SPLIT>(k_row, u, kv);
#pragma unroll
                for (int q = 0; q < CE_QG; ++q) {
                    float qv[8];
                    cq_unit<SPLIT>(ce_q + q * row4, u, qv);
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[q] = fmaf(qv[e], kv[e], acc[q]);
                }
            }
        }
        int bad = 0;
#pragma unroll
        for (int q = 0; q < CE_QG; ++q) {
            float v = acc[q];
            v = v + __shfl_xor(v, 1);                              // a0 + a1 | a2 + a3 (the same bits on both lanes of a pair)
            v = v + __shfl_xor(v, 2);
            const float sv = a.theta * v;
            if (ok && sub == 0 && q < ng) {
                s_out[(size_t)(k0 + q) * a.ld_s] = sv;
                bad |= !isfinite(sv);
            }
        }
        if (bad && a.flags) atomicOr(a.flags, 8);
    }
}

struct CellPatchArgs {
    float *s, *edge;
    const int *words, *count, *idx, *cnt, *sent_len, *wl, *wl_off, *wl_idx, *wl_out, *live_base;
    const float *part;
    double *lse;
    int *flags;
    int ld_s, cap, n_src, N, frame, beam, ld_part, n_parts, wl_base;
    double log1m, log_rho;             // log(1 - lambda), log(lambda / (1 - lambda))
};

__global__ void __launch_bounds__(CE_THREADS) cache_cell_patch_kernel(const CellPatchArgs a) {
    extern __shared__ __attribute__((aligned(16))) double ce_lds[];   // int [n_pad] words | [beam] L | float [beam] Z
    const int j = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (a.frame >= a.sent_len[j]) return;                          // (block-uniform, as every return below)
    const int kcnt = min(a.cnt[j], a.beam);
    if (kcnt <= 0) return;
    int r;
    const int n = ce_window(a.idx, a.count, j, a.n_src, a.cap, a.N, r);
    const int n_pad = (min(a.cap, a.N) + 3) & ~3;
    int *sh_w = reinterpret_cast<int *>(ce_lds);                   // (n_pad % 4 == 0: the 16-byte reads of the words, L's 8 bytes)
    double *sh_L = reinterpret_cast<double *>(sh_w + n_pad);
    float *sh_z = reinterpret_cast<float *>(sh_L + a.beam);

    // ---- the cell's log-normalisers: the beam step's fused fold, by one wave, whether the sentence has a window or not (the next
    //      beam step reads lse: it runs unfused)
    if (a.part) {
        if (wv == 0) {
            jlm_beam_state st = {};
            st.lse_part = a.part;
            st.ld_part = a.ld_part;
            st.n_parts = a.n_parts;
            st.flags = a.flags;
            beam_fold_parts(st, lane, kcnt, a.live_base[j], sh_L, a.lse + (size_t)j * a.beam);
        }
    } else {
        for (int k = tid; k < kcnt; k += CE_THREADS) sh_L[k] = 0.0;
    }
    if (n <= 0) return;                                            // an empty window: the cell's edge logits keep their bits

    for (int i = tid; i < ((n + 3) & ~3); i += CE_THREADS) sh_w[i] = i < n ? a.words[(size_t)(a.cap - n + i) * a.n_src + r] : -1;
    // ---- per slot: max, e_i over s, Z
    for (int k = wv; k < kcnt; k += CE_WAVES) {
        float *srow = a.s + ((size_t)j * a.beam + k) * a.ld_s;
        float mx = -INFINITY;
        int bad = 0;
        for (int i = lane; i < n; i += 64) {
            const float v = srow[i];
            mx = fmaxf(mx, v);
            bad |= !isfinite(v);
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            mx = fmaxf(mx, __shfl_xor(mx, off));
            bad |= __shfl_xor(bad, off);
        }
        if (bad) {                                                 // (wave-uniform) a score that is not finite: the slot keeps its logits
            if (lane == 0) {
                sh_z[k] = 0.0f;
                if (a.flags) atomicOr(a.flags, 8);
            }
            continue;
        }
        float z = 0.0f;
        for (int i = lane; i < n; i += 64) {
            const float e = expf(srow[i] - mx);
            srow[i] = e;
            z += e;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) z = z + __shfl_xor(z, off);
        if (lane == 0) sh_z[k] = z;                                // (>= 1: the maximum's own term)
    }
    __syncthreads();                                               // L, the words, Z and the e_i in s: visible to every thread

    const int l = a.wl_base + a.wl_idx[j];                         // the cell's list, as jlm_edge_logits finds it
    const int off0 = a.wl_off[l], J = a.wl_off[l + 1] - off0;
    const float *e_rows = a.s + (size_t)j * a.beam * a.ld_s;
    for (int p = tid; p < J; p += CE_THREADS) {
        const int w = a.wl[off0 + p];
        float *e_out = a.edge + (size_t)a.wl_out[off0 + p] * a.beam;
        int n_match = 0;
        for (int k0 = 0; k0 < kcnt; k0 += CE_QG) {
            float M[CE_QG];
#pragma unroll
            for (int q = 0; q < CE_QG; ++q) M[q] = 0.0f;
            if (k0 == 0 || n_match > 0) {
                for (int i0 = 0; i0 < n; i0 += 4) {
                    const int4 w4 = *reinterpret_cast<const int4 *>(sh_w + i0);
                    const int wi[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
                    for (int t = 0; t < 4; ++t)
                        if (wi[t] == w && i0 + t < n) {
                            n_match += k0 == 0;
#pragma unroll
                            for (int q = 0; q < CE_QG; ++q)
                                if (k0 + q < kcnt) M[q] += e_rows[(size_t)(k0 + q) * a.ld_s + i0 + t];
                        }
                }
            }
#pragma unroll
            for (int q = 0; q < CE_QG; ++q) {
                const int k = k0 + q;
                if (k >= kcnt) break;
                const float Z = sh_z[k];
                if (!(Z > 0.0f)) continue;
                const double y = (double)e_out[k], L = sh_L[k];
                const double v = n_match > 0 ? L + a.log1m + jlm_logaddexp(y - L, (a.log_rho + log((double)M[q])) - log((double)Z))
                                             : y + a.log1m;
                e_out[k] = (float)v;
            }
        }
    }
}

// what both launchers refuse of the window and the scratch: -1, or 0
int ce_refuse_window(int cap, int n_src, int N, int ld_s, int n_sent, int beam, int frame) {
    if (n_sent < 0 || n_src < 0 || frame < 0 || beam < 1 || beam > JLM_MAX_BEAM) return -1;
    if (N < 1 || N > JLM_CACHE_MIX_MAX_N || cap < 1 || ld_s < (cap < N ? cap : N)) return -1;
    if (n_sent > 65535) return -1;
    return 0;
}

}  // namespace

// the refusals of jlm_cache_cell_query on their own (jlm_decode_frames asks before its first launch): -1, or 0
int jlm_cache_cell_query_refuse(const void *h, int H, int split, float h_scale, const int *g0, const int *cnt, const int *sent_len, int frame,
                                int n_sent, int beam, const void *hist, const int *count, int cap, int n_src, const int *idx, int N,
                                float theta, const float *s, int ld_s, const int *flags) {
    if (int rc = ce_refuse_window(cap, n_src, N, ld_s, n_sent, beam, frame)) return rc;
    if (H <= 0 || H % 32 != 0) return -1;                          // what jlm_lstm_step / jlm_lstm_step_xg accept
    if ((long long)CE_QG * H * 4 > 65536) return -1;               // the staged query rows: 64 KB of LDS at most (H <= 2048)
    if (!(theta >= 0.0f) || !isfinite(theta)) return -1;
    if (split && !(h_scale > 0.0f && isfinite(h_scale))) return -1;
    if (n_sent == 0) return 0;
    if (!h || !g0 || !cnt || !sent_len || !hist || !count || !idx || !s) return -1;
    if ((((uintptr_t)h | (uintptr_t)hist) & 15) != 0 || (((uintptr_t)s | (uintptr_t)flags) & 3) != 0) return -1;
    return 0;
}

// the refusals of jlm_cache_cell_patch on their own
int jlm_cache_cell_patch_refuse(const float *s, int ld_s, const int *words, const int *count, int cap, int n_src, const int *idx, int N,
                                float lam, const int *cnt, const int *sent_len, int frame, int n_sent, int beam, const int *wl,
                                const int *wl_off, const int *wl_idx, int wl_base, const int *wl_out, const float *edge, const float *part,
                                int ld_part, int n_parts, const int *live_base, const double *lse, const int *flags) {
    if (int rc = ce_refuse_window(cap, n_src, N, ld_s, n_sent, beam, frame)) return rc;
    if (!(lam > 0.0f && lam < 1.0f)) return -1;
    if (part && (!live_base || !lse || n_parts < 1 || ld_part < 1)) return -1;
    if (n_sent == 0) return 0;
    if (!s || !words || !count || !idx || !cnt || !sent_len || !wl || !wl_off || !wl_idx || wl_base < 0 || !wl_out || !edge) return -1;
    if ((((uintptr_t)s | (uintptr_t)edge | (uintptr_t)flags) & 3) != 0 || ((uintptr_t)part & 7) != 0 || ((uintptr_t)lse & 7) != 0) return -1;
    return 0;
}

extern "C" int jlm_cache_cell_query(const void *h, int H, int split, float h_scale, const int *g0, const int *cnt, const int *sent_len,
                                    int frame, int n_sent, int beam, const void *hist, const int *count, int cap, int n_src, const int *idx,
                                    int N, float theta, float *s, int ld_s, int *flags, void *stream) {
    if (int rc = jlm_cache_cell_query_refuse(h, H, split, h_scale, g0, cnt, sent_len, frame, n_sent, beam, hist, count, cap, n_src, idx, N,
                                             theta, s, ld_s, flags))
        return rc;
    if (n_sent == 0) return 0;
    CellQueryArgs a;
    a.h = (const uint4 *)h; a.hist = (const uint4 *)hist; a.g0 = g0; a.cnt = cnt; a.sent_len = sent_len; a.count = count; a.idx = idx;
    a.s = s; a.flags = flags; a.H = H; a.frame = frame; a.beam = beam; a.cap = cap; a.n_src = n_src; a.N = N; a.ld_s = ld_s;
    a.theta = split ? theta / (h_scale * h_scale) : theta;
    const int n_max = cap < N ? cap : N;
    const dim3 grid((n_max + CE_KEYS - 1) / CE_KEYS, n_sent);
    const size_t lds = (size_t)CE_QG * H * 4;                      // 16 KB at H = 512
    if (split)
        cache_cell_query_kernel<true><<<grid, dim3(4 * CE_KEYS), lds, (hipStream_t)stream>>>(a);
    else
        cache_cell_query_kernel<false><<<grid, dim3(4 * CE_KEYS), lds, (hipStream_t)stream>>>(a);
    return (int)hipGetLastError();
}

extern "C" int jlm_cache_cell_patch(float *s, int ld_s, const int *words, const int *count, int cap, int n_src, const int *idx, int N,
                                    float lam, const int *cnt, const int *sent_len, int frame, int n_sent, int beam, const int *wl,
                                    const int *wl_off, const int *wl_idx, int wl_base, const int *wl_out, float *edge, const float *part,
                                    int ld_part, int n_parts, const int *live_base, double *lse, int *flags, void *stream) {
    if (int rc = jlm_cache_cell_patch_refuse(s, ld_s, words, count, cap, n_src, idx, N, lam, cnt, sent_len, frame, n_sent, beam, wl, wl_off,
                                             wl_idx, wl_base, wl_out, edge, part, ld_part, n_parts, live_base, lse, flags))
        return rc;
    if (n_sent == 0) return 0;
    CellPatchArgs a;
    a.s = s; a.edge = edge; a.words = words; a.count = count; a.idx = idx; a.cnt = cnt; a.sent_len = sent_len; a.wl = wl; a.wl_off = wl_off; a.wl_idx = wl_idx; a.wl_base = wl_base;
    a.wl_out = wl_out; a.live_base = live_base; a.part = part; a.lse = lse; a.flags = flags; a.ld_s = ld_s; a.cap = cap; a.n_src = n_src;
    a.N = N; a.frame = frame; a.beam = beam; a.ld_part = ld_part; a.n_parts = n_parts;
    a.log1m = log1p(-(double)lam);
    a.log_rho = log((double)lam) - log1p(-(double)lam);
    const int n_pad = ((cap < N ? cap : N) + 3) & ~3;
    const size_t lds = (size_t)beam * 8 + (size_t)n_pad * 4 + (size_t)beam * 4;     // 28 KB at most (beam 1 024, N 4 096)
    cache_cell_patch_kernel<<<dim3(n_sent), dim3(CE_THREADS), lds, (hipStream_t)stream>>>(a);
    return (int)hipGetLastError();
}
