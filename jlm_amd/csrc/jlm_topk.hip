// jlm_topk.hip -- the two kernels of a beam-search frame over materialised f32 logits (jlm_complete_frames, include/jlm_hip.h;
// jlm_decode.hip enqueues them after the logit GEMMs): topk_rows_kernel, the k best words of every row with their -log p, and
// beam_merge_kernel, the per-prompt merge of those lists into the next beam.  What the reference's find_top_N (decoder/model.py:25-26)
// does with an argsort of one host-side distribution, and the n-best continuation it has no loop for.
//
// topk_rows_kernel -- one workgroup of TK_WAVES waves per row, the row read ONCE in sample_rows_kernel's layout (16-byte chunks, an
// "iteration" = 64 consecutive chunks, wave w owns the contiguous iterations [w * ipw, (w + 1) * ipw): wave spans in word order).
//   lse   csrc/jlm_row_lse.h, the definition the cache and n-gram mix kernels share: per lane a running max m and an f64 sum of f32
//         expf(y - m), moved by groups of TK_UNROLL chunks (rl_group's statements, written out below on the chunks loaded for the
//         lists), an xor-tree over the wave (rl_wave_merge), waves merged in order (rl_block_merge).  A NaN logit makes the sum NaN:
//         flagged.
//   top-k per wave a candidate list in LDS (TK_CAP entries).  Until it holds k entries every word is appended; after that only words
//         ABOVE the k-th entry's logit: the span is read in ascending id order, so a later word equal to it has a higher id and
//         ranks below it.  Appends are ballot-compacted; when the next iteration could overflow the list, the wave selects its
//         top k (tk_select: k rounds of a wave-wide argmax over the entries, lanes caching their best) and raises the threshold.
//   Ranking: y descending, then id ascending -- the greedy draw's rule (sample_rows_kernel).  At the end wave 0 selects the row's
//   top k from the waves' lists; nll = (m + log S) - y in f64 (self_norm: -y).  A non-finite max or sum: *flags |= 1, ids -1, nll NaN.
//
//   topk_rows_masked_kernel is the same body (topk_row<SELF_NORM, MASKED = 1>) with each row's candidates restricted to a word set:
//   a bit mask per set, four bits per 16-byte chunk, read beside the logits.  The lse is untouched by the mask; a set with fewer than
//   k rankable words pads its list with (-1, +inf).  A row of set -1 loads no mask and is the unmasked row bit for bit.
//
// beam_merge_kernel -- one wave per prompt, lane j = the previous beam's rank j.  A lane's candidates are its row's list in order
// (score = parent score + nll, f64: non-decreasing along the list), or, for a finished parent, one carry (score unchanged, word -1).
// B rounds: each lane offers its best remaining candidate by (score, word id) -- the list order, but where f64 rounding makes
// neighbours' scores equal the lower id first -- and the wave takes the offer with the smallest (score, lane).
#include "jlm_common.h"
#include "jlm_row_lse.h"

#define TK_WAVES RL_WAVES               // the row layout is csrc/jlm_row_lse.h's: its wave count and its group of chunks
#define TK_THREADS (64 * TK_WAVES)
#define TK_UNROLL RL_GROUP
#define TK_CAP 512                      // per-wave candidate list; >= JLM_TOPK_MAX + 4 * 64 (one iteration's appends)
#define TK_SLOTS (TK_CAP / 64)

static_assert(TK_CAP >= JLM_TOPK_MAX + 4 * 64, "a compacted list plus one iteration's appends must fit");
static_assert(TK_WAVES * JLM_TOPK_MAX <= TK_CAP, "wave 0's list takes every wave's top k");

__device__ __forceinline__ bool tk_better(float ya, int ia, float yb, int ib) { return ya > yb || (ya == yb && ia < ib); }

// the n entries of one wave's list (sy, si) -> its best min(k, n) in rank order at sy / si [0 ..).  Lane l owns slots l + 64 s.
// Entries are never NaN and ids are distinct, so exactly one lane holds each round's winner.
__device__ int tk_select(float *sy, int *si, int n, int k, int lane) {
    const int kk = min(k, n);
    unsigned removed = 0;
    float by = -INFINITY;
    int bi = 0x7fffffff, bs = -1;
    auto rescan = [&]() {
        by = -INFINITY; bi = 0x7fffffff; bs = -1;
#pragma unroll
        for (int s = 0; s < TK_SLOTS; ++s) {
            const int e = lane + 64 * s;
            if (e < n && !((removed >> s) & 1u)) {
                const float y = sy[e];
                const int i = si[e];
                if (tk_better(y, i, by, bi)) { by = y; bi = i; bs = s; }
            }
        }
    };
    rescan();
    float oy = -INFINITY;
    int oi = -1;
    for (int t = 0; t < kk; ++t) {
        float wy = by;
        int wi = bi;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const float y2 = __shfl_xor(wy, off);
            const int i2 = __shfl_xor(wi, off);
            if (tk_better(y2, i2, wy, wi)) { wy = y2; wi = i2; }
        }
        if (lane == t) { oy = wy; oi = wi; }
        if (bs >= 0 && bi == wi) { removed |= 1u << bs; rescan(); }
    }
    if (lane < kk) { sy[lane] = oy; si[lane] = oi; }    // one wave, in order: every read above precedes these writes
    return kk;
}

// One row.  MASKED: only the words whose bit is set in mrow (bit w & 31 of word w >> 5) enter the lists and the threshold test -- the
// max and the sum still run over every word, in the same order -- and a row with fewer than k rankable words pads its output with
// (-1, +inf) instead of flagging; mrow NULL is an unrestricted row: no mask is loaded and every branch below is the unmasked one.
// bad (MASKED only): the row's set index is out of range; the row is flagged.
template <int SELF_NORM, int MASKED>
__device__ __forceinline__ void topk_row(const float *__restrict__ y, int ld, int n_cols, int r, int k, const unsigned *__restrict__ mrow,
                                         bool bad, int *__restrict__ ids, double *__restrict__ nll, int ld_out, int *flags) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    __shared__ float s_y[TK_WAVES * TK_CAP];
    __shared__ int s_i[TK_WAVES * TK_CAP];
    __shared__ float s_m[TK_WAVES];
    __shared__ double s_s[TK_WAVES];
    __shared__ int s_n[TK_WAVES];
    float *sy = s_y + wv * TK_CAP;
    int *si = s_i + wv * TK_CAP;
    const f32x4 *row = reinterpret_cast<const f32x4 *>(y + (size_t)r * ld);
    const int n4 = (n_cols + 3) >> 2, n_it = (n4 + 63) >> 6;
    const int ipw = (n_it + TK_WAVES - 1) / TK_WAVES;
    const int it0 = wv * ipw, it1 = min(it0 + ipw, n_it);
    const unsigned long long below = (1ull << lane) - 1ull;

    float m = -INFINITY;
    double s = 0.0;
    int cnt = 0;                                         // wave-uniform: entries in the list
    bool full = false;                                   // the list held k entries at its last selection
    float th = -INFINITY;                                // then: the k-th entry's logit
    for (int it = it0; it < it1; it += TK_UNROLL) {
        f32x4 v[TK_UNROLL];
        unsigned mb[TK_UNROLL];
#pragma unroll
        for (int u = 0; u < TK_UNROLL; ++u) {
            const int c = (it + u) * 64 + lane;
            v[u] = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
            if (it + u < it1 && c < n4) v[u] = row[c];
            if (MASKED) {                                // the chunk's four bits sit in one word (its first word id is 4 c), which is
                mb[u] = 0;                               // read with the logits and only where they are: 4 c < n_cols <= 32 * ld_mask
                if (mrow && it + u < it1 && c < n4) mb[u] = mrow[c >> 3] >> (4 * (c & 7));
            }
        }
        if (!SELF_NORM) {
            // rl_group's statements (csrc/jlm_row_lse.h), written out: called as a function, the compiler no longer shares the sixteen
            // word-bound tests between this sum and the list code below: 30 instructions more, and the selection of
            // tools/complete_bench.py 1.1 to 3.1 % slower than the parent at four of six shapes, outside the parent's own spread
            // (profiles/shared_arith_bench_ab.txt, set 1 against set 2).  A COPY: a change to rl_group is made
            // here too.  tests/row_lse_pin.py holds it to rl_row's L on the device, to float32 resolution.
            float cm = -INFINITY;
#pragma unroll
            for (int u = 0; u < TK_UNROLL; ++u)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (4 * ((it + u) * 64 + lane) + j < n_cols) cm = fmaxf(cm, v[u][j]);
            if (cm > m) { s = rl_rescale(s, m, cm); m = cm; }
            const float me = m > -INFINITY ? m : 0.0f;
#pragma unroll
            for (int u = 0; u < TK_UNROLL; ++u)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (4 * ((it + u) * 64 + lane) + j < n_cols) s += (double)expf(v[u][j] - me);
        } else {
#pragma unroll
            for (int u = 0; u < TK_UNROLL; ++u)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (4 * ((it + u) * 64 + lane) + j < n_cols) m = fmaxf(m, v[u][j]);
        }
#pragma unroll
        for (int u = 0; u < TK_UNROLL; ++u) {
            if (it + u >= it1) break;                    // wave-uniform
            const int w0 = 4 * ((it + u) * 64 + lane);
            bool p[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) p[j] = w0 + j < n_cols && (full ? v[u][j] > th : v[u][j] == v[u][j]);
            if (MASKED && mrow) {                        // block-uniform
#pragma unroll
                for (int j = 0; j < 4; ++j) p[j] = p[j] && ((mb[u] >> j) & 1u);
            }
            if (__ballot(p[0] | p[1] | p[2] | p[3]) == 0ull) continue;
            if (cnt + 4 * 64 > TK_CAP) {
                cnt = tk_select(sy, si, cnt, k, lane);
                full = cnt >= k;
                if (full) {
                    th = sy[k - 1];
#pragma unroll
                    for (int j = 0; j < 4; ++j) p[j] = p[j] && v[u][j] > th;
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned long long b = __ballot(p[j]);
                if (p[j]) {
                    const int e = cnt + __popcll(b & below);
                    sy[e] = v[u][j];
                    si[e] = w0 + j;
                }
                cnt += __popcll(b);
            }
        }
    }
    if (cnt > 0) cnt = tk_select(sy, si, cnt, k, lane);
    if (!SELF_NORM) {
        rl_wave_merge(m, s);
    } else {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
    }
    if (lane == 0) { s_m[wv] = m; s_s[wv] = s; s_n[wv] = cnt; }
    __syncthreads();
    if (wv != 0) return;
    float M;
    double S;
    rl_block_merge(s_m, s_s, M, S);                      // (SELF_NORM: every s_s is 0 and S is not used)
    int total = s_n[0];
    for (int w = 1; w < TK_WAVES; ++w) {                 // the other waves' lists behind wave 0's
        if (lane < s_n[w]) { s_y[total + lane] = s_y[w * TK_CAP + lane]; s_i[total + lane] = s_i[w * TK_CAP + lane]; }
        total += s_n[w];
    }
    const int kk = total > 0 ? tk_select(s_y, s_i, total, k, lane) : 0;
    const bool padded = MASKED && mrow;                  // a restricted row may hold fewer than k rankable words
    const bool ok = M > -INFINITY && M < INFINITY && (kk == k || padded) && (SELF_NORM || (S > 0.0 && S < INFINITY)) && !(MASKED && bad);
    if (!ok) {
        if (lane == 0 && flags) atomicOr(flags, 1);
        if (lane < k) { ids[(size_t)r * ld_out + lane] = -1; nll[(size_t)r * ld_out + lane] = __longlong_as_double(0x7ff8000000000000LL); }
        return;
    }
    if (lane < (MASKED ? kk : k)) {                      // (not MASKED: kk == k here)
        const float yv = s_y[lane];
        ids[(size_t)r * ld_out + lane] = s_i[lane];
        nll[(size_t)r * ld_out + lane] = SELF_NORM ? -(double)yv : ((double)M + log(S)) - (double)yv;
    } else if (MASKED && lane < k) {
        ids[(size_t)r * ld_out + lane] = -1;
        nll[(size_t)r * ld_out + lane] = INFINITY;
    }
}

template <int SELF_NORM>
__global__ __launch_bounds__(TK_THREADS) void topk_rows_kernel(const float *__restrict__ y, int ld, int n_cols, int n_rows, int k,
                                                               int *__restrict__ ids, double *__restrict__ nll, int ld_out, int *flags) {
    const int r = blockIdx.x;
    if (r >= n_rows) return;
    topk_row<SELF_NORM, 0>(y, ld, n_cols, r, k, nullptr, false, ids, nll, ld_out, flags);
}

// topk_rows_kernel with row r restricted to the words of set row_set[r] of mask [n_sets][ld_mask] (-1: unrestricted)
template <int SELF_NORM>
__global__ __launch_bounds__(TK_THREADS) void topk_rows_masked_kernel(const float *__restrict__ y, int ld, int n_cols, int n_rows, int k,
                                                                      const unsigned *__restrict__ mask, int ld_mask, int n_sets,
                                                                      const int *__restrict__ row_set, int *__restrict__ ids,
                                                                      double *__restrict__ nll, int ld_out, int *flags) {
    const int r = blockIdx.x;
    if (r >= n_rows) return;
    const int s = row_set[r];                            // block-uniform
    const bool bad = s < -1 || s >= n_sets;              // (the torch op refuses it on the host; a C caller's is flagged, never indexed)
    topk_row<SELF_NORM, 1>(y, ld, n_cols, r, k, s >= 0 && !bad ? mask + (size_t)s * ld_mask : nullptr, bad, ids, nll, ld_out, flags);
}

extern "C" int jlm_topk_rows(const float *y, int ld_y, int n_cols, int n_rows, int k, int self_norm, int *ids, double *nll, int ld_out,
                             int *flags, void *stream) {
    if (n_cols < 1 || ld_y % 4 != 0 || ld_y < ((n_cols + 3) & ~3) || ((uintptr_t)y & 15) != 0) return -1;
    if (k < 1 || k > JLM_TOPK_MAX || k > n_cols || ld_out < k || !ids || !nll) return -1;
    if (n_rows <= 0) return 0;
    if (self_norm)
        hipLaunchKernelGGL(topk_rows_kernel<1>, dim3(n_rows), dim3(TK_THREADS), 0, (hipStream_t)stream, y, ld_y, n_cols, n_rows, k, ids,
                           nll, ld_out, flags);
    else
        hipLaunchKernelGGL(topk_rows_kernel<0>, dim3(n_rows), dim3(TK_THREADS), 0, (hipStream_t)stream, y, ld_y, n_cols, n_rows, k, ids,
                           nll, ld_out, flags);
    JLM_LAUNCH_CHECK();
    return 0;
}

extern "C" int jlm_topk_rows_masked(const float *y, int ld_y, int n_cols, int n_rows, int k, int self_norm, const unsigned *mask,
                                    int ld_mask, int n_sets, const int *row_set, int *ids, double *nll, int ld_out, int *flags,
                                    void *stream) {
    if (n_cols < 1 || ld_y % 4 != 0 || ld_y < ((n_cols + 3) & ~3) || ((uintptr_t)y & 15) != 0) return -1;
    if (k < 1 || k > JLM_TOPK_MAX || k > n_cols || ld_out < k || !ids || !nll) return -1;
    if (n_sets < 0 || !row_set || (n_sets > 0 && (!mask || ld_mask < (n_cols + 31) / 32))) return -1;
    if (n_rows <= 0) return 0;
    if (self_norm)
        hipLaunchKernelGGL(topk_rows_masked_kernel<1>, dim3(n_rows), dim3(TK_THREADS), 0, (hipStream_t)stream, y, ld_y, n_cols, n_rows, k,
                           mask, ld_mask, n_sets, row_set, ids, nll, ld_out, flags);
    else
        hipLaunchKernelGGL(topk_rows_masked_kernel<0>, dim3(n_rows), dim3(TK_THREADS), 0, (hipStream_t)stream, y, ld_y, n_cols, n_rows, k,
                           mask, ld_mask, n_sets, row_set, ids, nll, ld_out, flags);
    JLM_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// beam_merge_kernel (see the file's header).  Candidate rows: first ? row p (the prompt's one distribution, parent score 0) :
// rows p * B + j, j < B.  Writes rank i of prompt p at row q = p * B + i: the next frame's word / prev row / score / finished, and the
// back-pointers bp_*[q] (parent rank, word or -1 for a carry, nll or 0).  In place: every lane reads its parent's score and finished
// flag before any lane writes (one wave).
__device__ __forceinline__ bool bm_less(double sa, int la, double sb, int lb) { return sa < sb || (sa == sb && la < lb); }

__global__ __launch_bounds__(64) void beam_merge_kernel(const int *__restrict__ cand_ids, const double *__restrict__ cand_nll, int B,
                                                        int n_prompts, int first, int stop_id, int *word, int *prev, double *score,
                                                        int *finished, int *__restrict__ bp_parent, int *__restrict__ bp_word,
                                                        double *__restrict__ bp_nll) {
    const int p = blockIdx.x, lane = threadIdx.x;
    if (p >= n_prompts) return;
    const bool live = first ? lane == 0 : lane < B;
    const int src = first ? p : p * B + lane;
    double ps = 0.0;
    bool fin = false;
    if (live && !first) { ps = score[src]; fin = finished[src] != 0; }
    // the prompt's lists (rows contiguous: row p, or rows p * B .. p * B + B - 1) into LDS first: the rounds' reads are then LDS hits
    __shared__ int l_id[JLM_TOPK_MAX * JLM_TOPK_MAX];
    __shared__ double l_nll[JLM_TOPK_MAX * JLM_TOPK_MAX];
    const size_t base = (size_t)(first ? p : p * B) * B;
    for (int i = lane; i < (first ? 1 : B) * B; i += 64) { l_id[i] = cand_ids[base + i]; l_nll[i] = cand_nll[base + i]; }
    __syncthreads();
    const int *ci = l_id + (first ? 0 : lane * B);
    const double *cn = l_nll + (first ? 0 : lane * B);
    unsigned long long taken = 0;
    int ptr = live ? 0 : B;                              // the first candidate not taken (a carry: 0 until taken, then B)
    double hs = INFINITY, hn = 0.0;
    int hw = -1, hslot = -1;
    auto head = [&]() {
        hs = INFINITY; hn = 0.0; hw = -1; hslot = -1;
        if (ptr >= B) return;
        if (fin) { hs = ps; hslot = 0; return; }
        hslot = ptr;
        hn = cn[ptr];
        hw = ci[ptr];
        hs = ps + hn;
        for (int i = ptr + 1; i < B; ++i) {              // equal scores (rounding): the lower id first
            if ((taken >> i) & 1ull) continue;
            const double ni = cn[i];
            if (!(ps + ni == hs)) break;
            const int wi = ci[i];
            if (wi < hw) { hslot = i; hn = ni; hw = wi; }
        }
    };
    head();
    double o_s = 0.0, o_n = 0.0;
    int o_w = -1, o_p = 0;
    for (int t = 0; t < B; ++t) {
        double ks = hslot < 0 ? INFINITY : (hs != hs ? INFINITY : hs);    // a NaN score (flagged row) ranks last among live offers
        int kl = hslot < 0 ? 64 : lane;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const double s2 = __shfl_xor(ks, off);
            const int l2 = __shfl_xor(kl, off);
            if (bm_less(s2, l2, ks, kl)) { ks = s2; kl = l2; }
        }
        const int wl = kl & 63;                          // (kl < 64: B <= 64 candidates remain in every round)
        const double ws = __shfl(hs, wl), wn = __shfl(hn, wl);
        const int ww = __shfl(hw, wl);
        if (lane == t) { o_s = ws; o_n = wn; o_w = ww; o_p = wl; }
        if (lane == wl) {
            if (fin) ptr = B;
            else {
                taken |= 1ull << hslot;
                while (ptr < B && ((taken >> ptr) & 1ull)) ++ptr;
            }
            head();
        }
    }
    if (lane >= B) return;
    const int q = p * B + lane;
    const bool fin_new = o_w < 0 || (stop_id >= 0 && o_w == stop_id);
    score[q] = o_s;
    finished[q] = fin_new ? 1 : 0;
    word[q] = o_w >= 0 ? o_w : (stop_id >= 0 ? stop_id : 0);    // a carry (or a flagged row's -1) steps a valid word
    prev[q] = first ? p : p * B + o_p;
    bp_parent[q] = o_p;
    bp_word[q] = o_w;
    bp_nll[q] = o_n;
}

extern "C" int jlm_beam_merge(const int *cand_ids, const double *cand_nll, int beam, int n_prompts, int first, int stop_id, int *word,
                              int *prev, double *score, int *finished, int *bp_parent, int *bp_word, double *bp_nll, void *stream) {
    if (beam < 1 || beam > JLM_TOPK_MAX || !cand_ids || !cand_nll || !word || !prev || !score || !finished || !bp_parent || !bp_word ||
        !bp_nll)
        return -1;
    if (n_prompts <= 0) return 0;
    hipLaunchKernelGGL(beam_merge_kernel, dim3(n_prompts), dim3(64), 0, (hipStream_t)stream, cand_ids, cand_nll, beam, n_prompts, first,
                       stop_id, word, prev, score, finished, bp_parent, bp_word, bp_nll);
    JLM_LAUNCH_CHECK();
    return 0;
}
