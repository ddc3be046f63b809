// jlm_memory_edge.hip -- a memory of (hidden state, next word) pairs inside the decode's frame loop (include/jlm_hip.h
// jlm_memory_gather_rows / jlm_memory_cell_patch): the mass of the K nearest entries of every hypothesis row on
// every lattice edge leaving a frame, as a rewrite of the edge-logit buffer the next beam step reads.  Unlike the continuous cache
// (csrc/jlm_cache_edge.hip), whose window belongs to the sentence, the retrieved list belongs to the ROW: every slot of a cell has its
// own words.
//
// memory_gather_rows_kernel -- the frame's live rows, scattered through the state pool, into the contiguous query rows jlm_memory_topk
// reads: 16-byte loads and stores, one record a thread per trip, rows past the live count untouched.
//
// memory_cell_patch_kernel -- one workgroup of 256 threads per sentence.  Wave 0 folds the cell's normaliser slices into lse with the
// beam step's own fold (csrc/jlm_beam_fold.h); wave w then takes the slots w, w + 4, ... one at a time: the maximum, e_i and Z in
// cache_cell_patch_kernel's fixed tree (lane l owns i = l, l + 64, ... ascending, an xor tree), the slot's words and e_i staged in the
// wave's own slice of LDS (8 bytes an entry: 8 KiB a wave at K = 1 024, whatever the beam); then lane p takes the positions p, p + 64,
// ... of the cell's word list, walks the list four words a trip (one 16-byte LDS read at one address a wave: a broadcast), sums M in
// ascending i and rewrites the slot's edge logit of the position in f64 -- cache_cell_patch_kernel's arithmetic, operation for
// operation, restated here (tests/test_gpu_memory_edge.py holds the two together bit for bit).  L is read back from lse, which the
// fold wrote: nothing in LDS is sized by the beam.
#include <math.h>
#include "jlm_common.h"
#include "jlm_beam_fold.h"

namespace {

constexpr int ME_THREADS = 256;
constexpr int ME_WAVES = ME_THREADS / 64;

struct GatherArgs {
    const uint4 *h;
    uint4 *out;
    const int *rows, *n_dev;
    long long n_pool_rows;
    int row4, n_rows_max;
};

__global__ void __launch_bounds__(ME_THREADS) memory_gather_rows_kernel(const GatherArgs a) {
    const int n = a.n_dev ? min(max(*a.n_dev, 0), a.n_rows_max) : a.n_rows_max;
    const long long total = (long long)n * a.row4;
    for (long long t = (long long)blockIdx.x * ME_THREADS + threadIdx.x; t < total; t += (long long)gridDim.x * ME_THREADS) {
        const int i = (int)(t / a.row4), c = (int)(t - (long long)i * a.row4);
        const int g = a.rows[i];
        if (g < 0 || g >= a.n_pool_rows) continue;                 // (a row index outside the pool: nothing is read)
        a.out[(size_t)i * a.row4 + c] = a.h[(size_t)g * a.row4 + c];
    }
}

struct PatchArgs {
    const float *s, *part;
    float *edge;
    const int *ret_words, *cnt, *sent_len, *wl, *wl_off, *wl_idx, *wl_out, *live_base;
    double *lse;
    int *flags;
    int ld_s, n_rows, n_q, k_pad, frame, beam, ld_part, n_parts, wl_base;
    double log1m, log_rho;             // log(1 - lambda), log(lambda / (1 - lambda))
};

__global__ void __launch_bounds__(ME_THREADS) memory_cell_patch_kernel(const PatchArgs a) {
    extern __shared__ __attribute__((aligned(16))) int me_lds[];   // per wave: int [k_pad] words | float [k_pad] e
    const int j = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (a.frame >= a.sent_len[j]) return;                          // (block-uniform, as every return below)
    const int kcnt = min(a.cnt[j], a.beam);
    if (kcnt <= 0) return;
    const int base = a.live_base[j];
    double *lse_j = a.lse + (size_t)j * a.beam;

    // ---- the cell's log-normalisers: the beam step's fused fold, by one wave (the next beam step reads lse: it runs unfused)
    if (a.part) {
        if (wv == 0) {
            jlm_beam_state st = {};
            st.lse_part = a.part;
            st.ld_part = a.ld_part;
            st.n_parts = a.n_parts;
            st.flags = a.flags;
            beam_fold_parts(st, lane, kcnt, base, lse_j, lse_j);
        }
        __syncthreads();                                           // lse of the cell: visible to every wave
    }

    int *sh_w = me_lds + (size_t)wv * 2 * a.k_pad;                 // (k_pad % 4 == 0: the 16-byte reads of the words)
    float *sh_e = reinterpret_cast<float *>(sh_w + a.k_pad);
    const int n = a.n_q, n_pad = (n + 3) & ~3;
    const int l = a.wl_base + a.wl_idx[j];                         // the cell's list, as jlm_edge_logits finds it
    const int off0 = a.wl_off[l], J = a.wl_off[l + 1] - off0;
    for (int k = wv; k < kcnt; k += ME_WAVES) {                    // (everything in here is wave-uniform but the positions)
        const int c = base + k;                                    // the slot's compact row: its scores and its words
        if (c < 0 || c >= a.n_rows) continue;
        const float *srow = a.s + (size_t)c * a.ld_s;
        // ---- max, e_i, Z
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
        if (bad) {                                                 // a score that is not finite: the slot keeps its logits
            if (lane == 0 && a.flags) atomicOr(a.flags, 8);
            continue;
        }
        // (the lanes of the previous slot's walk have left the wave's slice: one wave, program order; the fences keep the compiler to it)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        float z = 0.0f;
        for (int i = lane; i < n_pad; i += 64) {
            float e = 0.0f;
            int w = -1;
            if (i < n) {
                e = expf(srow[i] - mx);
                w = a.ret_words[(size_t)i * a.n_rows + c];
                z += e;
            }
            sh_e[i] = e;
            sh_w[i] = w;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) z = z + __shfl_xor(z, off);      // (>= 1: the maximum's own term)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // ---- per position of the cell's word list: M in ascending i, the rewrite
        const double L = a.part ? lse_j[k] : 0.0;
        for (int p = lane; p < J; p += 64) {
            const int w = a.wl[off0 + p];
            float M = 0.0f;
            int n_match = 0;
            for (int i0 = 0; i0 < n; i0 += 4) {
                const int4 w4 = *reinterpret_cast<const int4 *>(sh_w + i0);
                const int wi[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    if (wi[t] == w && i0 + t < n) {
                        ++n_match;
                        M += sh_e[i0 + t];
                    }
            }
            float *e_out = a.edge + (size_t)a.wl_out[off0 + p] * a.beam + k;
            const double y = (double)*e_out;
            const double v = n_match > 0 ? L + a.log1m + jlm_logaddexp(y - L, (a.log_rho + log((double)M)) - log((double)z))
                                         : y + a.log1m;
            *e_out = (float)v;
        }
    }
}

}  // namespace

// the refusals of jlm_memory_gather_rows on their own (jlm_decode_frames asks before its first launch): -1, or 0
int jlm_memory_gather_rows_refuse(const void *h, int H, long long n_pool_rows, const int *rows, const int *n_dev, int n_rows_max,
                                  const void *out) {
    (void)n_dev;
    if (H <= 0 || H % 4 != 0 || n_pool_rows < 0 || n_rows_max < 0 || n_rows_max > 65535) return -1;
    if (n_rows_max == 0) return 0;
    if (!h || !rows || !out || n_pool_rows < 1) return -1;
    if ((((uintptr_t)h | (uintptr_t)out) & 15) != 0 || (((uintptr_t)rows | (uintptr_t)n_dev) & 3) != 0) return -1;
    return 0;
}

// the refusals of jlm_memory_cell_patch on their own
int jlm_memory_cell_patch_refuse(const float *s, int ld_s, const int *ret_words, int n_rows, int N, int K, float lam, const int *cnt,
                                 const int *sent_len, int frame, int n_sent, int beam, const int *wl, const int *wl_off, const int *wl_idx,
                                 int wl_base, const int *wl_out, const float *edge, const float *part, int ld_part, int n_parts,
                                 const int *live_base, const double *lse, const int *flags) {
    if (n_sent < 0 || frame < 0 || beam < 1 || beam > JLM_MAX_BEAM) return -1;
    if (N < 1 || K < 1 || K > JLM_MEMORY_TOPK_MAX || ld_s < K || n_rows < 1 || n_rows > 65535) return -1;
    if (n_sent > 65535) return -1;
    if (!(lam > 0.0f && lam < 1.0f)) return -1;
    if (part && (!lse || n_parts < 1 || ld_part < 1)) return -1;
    if (n_sent == 0) return 0;
    if (!s || !ret_words || !cnt || !sent_len || !wl || !wl_off || !wl_idx || wl_base < 0 || !wl_out || !edge || !live_base) return -1;
    if ((((uintptr_t)s | (uintptr_t)edge | (uintptr_t)flags | (uintptr_t)ret_words) & 3) != 0 || ((uintptr_t)part & 7) != 0 ||
        ((uintptr_t)lse & 7) != 0)
        return -1;
    return 0;
}

extern "C" int jlm_memory_gather_rows(const void *h, int H, long long n_pool_rows, const int *rows, const int *n_dev, int n_rows_max,
                                      void *out, void *stream) {
    if (int rc = jlm_memory_gather_rows_refuse(h, H, n_pool_rows, rows, n_dev, n_rows_max, out)) return rc;
    if (n_rows_max == 0) return 0;
    GatherArgs a;
    a.h = (const uint4 *)h; a.out = (uint4 *)out; a.rows = rows; a.n_dev = n_dev; a.n_pool_rows = n_pool_rows; a.row4 = H / 4;
    a.n_rows_max = n_rows_max;
    const long long total = (long long)n_rows_max * a.row4;
    const long long blocks = (total + ME_THREADS - 1) / ME_THREADS;
    memory_gather_rows_kernel<<<dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(ME_THREADS), 0, (hipStream_t)stream>>>(a);
    return (int)hipGetLastError();
}

extern "C" int jlm_memory_cell_patch(const float *s, int ld_s, const int *ret_words, int n_rows, int N, int K, float lam, const int *cnt,
                                     const int *sent_len, int frame, int n_sent, int beam, const int *wl, const int *wl_off,
                                     const int *wl_idx, int wl_base, const int *wl_out, float *edge, const float *part, int ld_part,
                                     int n_parts, const int *live_base, double *lse, int *flags, void *stream) {
    if (int rc = jlm_memory_cell_patch_refuse(s, ld_s, ret_words, n_rows, N, K, lam, cnt, sent_len, frame, n_sent, beam, wl, wl_off, wl_idx,
                                              wl_base, wl_out, edge, part, ld_part, n_parts, live_base, lse, flags))
        return rc;
    if (n_sent == 0) return 0;
    PatchArgs a;
    a.s = s; a.part = part; a.edge = edge; a.ret_words = ret_words; a.cnt = cnt; a.sent_len = sent_len; a.wl = wl; a.wl_off = wl_off;
    a.wl_idx = wl_idx; a.wl_out = wl_out; a.live_base = live_base; a.lse = lse; a.flags = flags; a.ld_s = ld_s; a.n_rows = n_rows;
    a.n_q = K < N ? K : N; a.k_pad = (a.n_q + 3) & ~3; a.frame = frame; a.beam = beam; a.ld_part = ld_part; a.n_parts = n_parts;
    a.wl_base = wl_base;
    a.log1m = log1p(-(double)lam);
    a.log_rho = log((double)lam) - log1p(-(double)lam);
    const size_t lds = (size_t)ME_WAVES * 2 * a.k_pad * 4;         // 32 KiB at most (K = 1 024), whatever the beam
    memory_cell_patch_kernel<<<dim3(n_sent), dim3(ME_THREADS), lds, (hipStream_t)stream>>>(a);
    return (int)hipGetLastError();
}
