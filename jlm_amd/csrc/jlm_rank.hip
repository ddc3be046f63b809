// jlm_rank.hip -- the rank of a given word in every row of materialised f32 logits (jlm_rank_rows, include/jlm_hip.h;
// jlm_decode.hip's jlm_rank_frames enqueues it after the logit GEMMs): where the word the user actually wrote stands among all
// words, among the words whose reading starts with what has been typed, and among its homophones.  The reference has find_top_N
// over one host-side distribution (decoder/model.py:25-26) and nothing that measures where the true word landed.
//
// rank_rows_kernel -- one workgroup of RK_WAVES waves per row, the order of topk_rows_kernel (jlm_topk.hip): a word ranks above the
// target t when its logit is greater, or equal with a lower id.  Every output is an integer count, so no order of summation enters.
//   level A   the row read once in 16-byte chunks, wave w of a trip owning 64 consecutive chunks: coalesced, RK_UNROLL loads in
//             flight.  A row whose target has a level list leaves "this word ranks above the target" as ONE BIT per word in LDS: the
//             wave's ballot of word j of its 64 chunks is two 32-bit words of plane j (bit c & 31 of word c >> 5 of plane w & 3 for
//             word w of chunk c = w >> 2), written by one lane each.  V / 8 bytes: 6 KB at V = 50 000.
//   levels    entry e of the target's level list is a span [lo, hi) of `ids` (the vocabulary sorted by (reading, id)); the threads
//             stride over it -- the index reads are coalesced -- and look each word's bit up in LDS, so a level costs 4 bytes of
//             global traffic per entry and nothing of the row.  (Gathering y[ids[i]] instead costs an L2 line per entry: measured at
//             V = 50 000 and 1 024 rows, 0.69 ms a launch against 0.04 ms for level A alone.)  One pass per level: a word's levels are
//             nested and shrink by the number of distinct kana a level, so the passes behind the first cost a few per cent of it, and
//             a pass needs no per-lane array of counters indexed at run time.
//             Rows of more than RK_BITMAP_MAX_COLS words (the bit planes would not fit 60 KB of LDS) gather from the row instead:
//             rank_rows_kernel<0>, the same counts.
//   sums      per level a wave's xor-tree, then one integer LDS add per wave; one barrier in front of the stores, thread c writes
//             column c: one writer per output, plain vector stores.
// A target outside [0, n_cols) or a NaN logit of the target ends the workgroup before anything is indexed by it (both block-uniform).
#include "jlm_common.h"

#define RK_WAVES 4
#define RK_THREADS (64 * RK_WAVES)
#define RK_UNROLL 4
#define RK_BITMAP_MAX_COLS 491520       // 4 planes x ceil(n4 / 64) x 8 bytes <= 60 KB

static_assert(JLM_RANK_MAX_LEVELS + 1 <= RK_THREADS, "thread c writes column c");

__device__ __forceinline__ int rk_wave_sum(int x) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off);
    return x;
}

// 32-bit words per bit plane: two per 64 chunks of 16 bytes
static inline int rk_plane_words(int n_cols) { return 2 * ((((n_cols + 3) >> 2) + 63) >> 6); }

template <int BITMAP>
__global__ __launch_bounds__(RK_THREADS) void rank_rows_kernel(const float *__restrict__ y, int ld, int n_cols, int n_rows_max,
                                                               const int *__restrict__ n_dev, const int *__restrict__ target,
                                                               const int *__restrict__ ids, int n_ids, const int *__restrict__ lv_off,
                                                               const int *__restrict__ lv_lo, const int *__restrict__ lv_hi, int n_levels,
                                                               int plane_words, int *__restrict__ rank, int *flags) {
    extern __shared__ unsigned s_bits[];                 // BITMAP: [4][plane_words]
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int n_rows = n_dev ? min(*n_dev, n_rows_max) : n_rows_max;
    if (r >= n_rows) return;
    int *out = rank + (size_t)r * (n_levels + 1);
    const int t = target[r];                             // block-uniform, as everything up to the scans
    const float *row = y + (size_t)r * ld;
    const bool inside = t >= 0 && t < n_cols;
    const float yt = inside ? row[t] : 0.0f;
    if (!inside || yt != yt) {
        if (tid <= n_levels) out[tid] = -1;
        if (tid == 0 && flags) atomicOr(flags, inside ? 1 : 2);
        return;
    }
    __shared__ int s_cnt[JLM_RANK_MAX_LEVELS + 1];
    if (tid <= n_levels) s_cnt[tid] = 0;
    int n_mine = 0, e0 = 0;
    if (lv_off) {
        e0 = lv_off[t];
        n_mine = min(max(lv_off[t + 1] - e0, 0), n_levels);
        if (e0 < 0) n_mine = 0;
    }
    const bool bits = BITMAP && n_mine > 0;              // block-uniform
    __syncthreads();

    // level A: a NaN compares false both ways and is never counted; the padding of the last chunk is no word
    const f32x4 *row4 = reinterpret_cast<const f32x4 *>(row);
    const int n4 = (n_cols + 3) >> 2;
    int cnt = 0;
    for (int base = 0; base < n4; base += RK_THREADS * RK_UNROLL) {
        f32x4 v[RK_UNROLL];
#pragma unroll
        for (int u = 0; u < RK_UNROLL; ++u) {
            const int c = base + u * RK_THREADS + tid;
            v[u] = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
            if (c < n4) v[u] = row4[c];
        }
#pragma unroll
        for (int u = 0; u < RK_UNROLL; ++u) {
            const int c_wave = base + u * RK_THREADS + wv * 64;          // the wave's first chunk: a multiple of 64
            if (c_wave >= n4) break;                                     // wave-uniform
            const int w0 = 4 * (c_wave + lane);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int w = w0 + j;
                const bool above = w < n_cols && (v[u][j] > yt || (v[u][j] == yt && w < t));
                cnt += above ? 1 : 0;
                if (bits) {
                    const unsigned long long b = __ballot(above);
                    if (lane < 2) s_bits[j * plane_words + (c_wave >> 5) + lane] = (unsigned)(b >> (32 * lane));
                }
            }
        }
    }
    cnt = rk_wave_sum(cnt);
    if (lane == 0) atomicAdd(&s_cnt[0], cnt);
    if (bits) __syncthreads();

    for (int e = 0; e < n_mine; ++e) {
        const int lo = max(lv_lo[e0 + e], 0), hi = min(lv_hi[e0 + e], n_ids);
        int k = 0;
        for (int i0 = lo + tid; i0 < hi; i0 += RK_THREADS * RK_UNROLL) {
            int w[RK_UNROLL];
#pragma unroll
            for (int u = 0; u < RK_UNROLL; ++u) {
                const int i = i0 + u * RK_THREADS;
                w[u] = i < hi ? ids[i] : -1;
            }
#pragma unroll
            for (int u = 0; u < RK_UNROLL; ++u) {        // an id outside the row is no word: nothing is read for it
                const bool ok = w[u] >= 0 && w[u] < n_cols;
                if (BITMAP) {
                    const unsigned word = ok ? s_bits[(w[u] & 3) * plane_words + (w[u] >> 7)] : 0u;
                    k += (int)((word >> ((w[u] >> 2) & 31)) & 1u);
                } else {
                    const float v = ok ? row[w[u]] : -INFINITY;
                    k += (v > yt || (v == yt && ok && w[u] < t)) ? 1 : 0;
                }
            }
        }
        k = rk_wave_sum(k);
        if (lane == 0) atomicAdd(&s_cnt[1 + e], k);
    }
    __syncthreads();
    if (tid <= n_levels) out[tid] = tid <= n_mine ? s_cnt[tid] : -1;
}

extern "C" int jlm_rank_rows(const float *y, int ld_y, int n_cols, int n_rows_max, const int *n_dev, const int *target, const int *ids,
                             int n_ids, const int *lv_off, const int *lv_lo, const int *lv_hi, int n_levels, int *rank, int *flags,
                             void *stream) {
    if (n_cols < 1 || ld_y % 4 != 0 || ld_y < ((n_cols + 3) & ~3) || ((uintptr_t)y & 15) != 0 || !y) return -1;
    if (n_levels < 0 || n_levels > JLM_RANK_MAX_LEVELS || !target || !rank) return -1;
    if (lv_off && (n_ids < 0 || !lv_lo || !lv_hi || (n_ids > 0 && !ids))) return -1;
    if (n_rows_max <= 0) return 0;
    const int pw = rk_plane_words(n_cols);
    if (n_cols <= RK_BITMAP_MAX_COLS)
        hipLaunchKernelGGL(rank_rows_kernel<1>, dim3(n_rows_max), dim3(RK_THREADS), lv_off ? (size_t)16 * pw : 0, (hipStream_t)stream, y, ld_y,
                           n_cols, n_rows_max, n_dev, target, ids, n_ids, lv_off, lv_lo, lv_hi, n_levels, pw, rank, flags);
    else
        hipLaunchKernelGGL(rank_rows_kernel<0>, dim3(n_rows_max), dim3(RK_THREADS), 0, (hipStream_t)stream, y, ld_y, n_cols, n_rows_max,
                           n_dev, target, ids, n_ids, lv_off, lv_lo, lv_hi, n_levels, pw, rank, flags);
    JLM_LAUNCH_CHECK();
    return 0;
}
