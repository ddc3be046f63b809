// jlm_score.hip -- the last kernel of a teacher-forced scoring step (jlm_score_frames, include/jlm_hip.h; jlm_decode.hip enqueues
// the step): per live row, the normaliser's (max, sum exp) slices folded into the log-normaliser, the target word's logit, and
// nll = lse - y accumulated in f64.  What the reference's LSTM_Model.evaluate reads off a materialised softmax one word at a time
// (decoder/model.py:200-206, 15-20, 117-119).
//
// A row is 8 lanes of a wave, 8 rows per wave, 32 per workgroup -- the beam step's fold layout (jlm_beam.hip, fused K6 tail):
//   fold    lane `sub` takes the slices p = sub, sub + 8, ...; three xor-shuffle steps merge the 8 partial (max, sum) pairs.
//           Same order and arithmetic as beam_step_kernel's fold, so a row's log-normaliser is the one the decode uses.
//   logit   the word-addressed logit of csrc/jlm_wordlist_dot.h (jlm_edge_logits): its wl_lookup and its wl_sum8 are called; the
//           fmaf chain between them is wl_dot's order (lane `sub`, chunks k4 = sub, sub + 8, ..., elements 0 .. 3) written out here,
//           because this kernel's T row is in global memory, not staged in LDS, and BOTH rows are requested whole before the first
//           use -- one round trip for the row pair.  + b2[w].
// Both equalities are held to the bit by tests/test_gpu_score_fold.py, which calls the kernel through jlm_score_fold.
// Latency-bound and tiny next to the step's three matrix kernels: one slice read per lane and slice row, one weight row per row.
#include "jlm_common.h"
#include "jlm_wordlist_dot.h"

#define SF_THREADS 256
#define SF_ROWS (SF_THREADS / 8)

template <int SELF_NORM>
__global__ __launch_bounds__(SF_THREADS) void score_fold_kernel(
    SegTable segs, const float *__restrict__ b2, const float *__restrict__ T, int ldt, const float2 *__restrict__ part, int ld_part,
    int n_parts, const int *__restrict__ target, const int *__restrict__ n_dev, int n_rows_max, double *__restrict__ nll_seq,
    double *__restrict__ nll_tok, int *flags) {
    const int sub = threadIdx.x & 7;
    const int r = blockIdx.x * SF_ROWS + (threadIdx.x >> 3);
    const int n = n_dev ? min(*n_dev, n_rows_max) : n_rows_max;
    // the 8 lanes of a row are live or not together; no lane leaves before the shuffles
    const bool live = r < n;
    float m = JLM_NEG_BIG;
    double sm = 0.0;
    if (!SELF_NORM) {
        auto fold = [&](const float2 v) {
            const float mm = fmaxf(m, v.x);
            sm = sm * (double)expf(m - mm) + (double)v.y * (double)expf(v.x - mm);
            m = mm;
        };
        if (live) {
            // four slices requested before the first is folded (same order as one at a time)
            int p = sub;
            for (; p + 24 < n_parts; p += 32) {
                float2 v[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = part[(size_t)(p + 8 * i) * ld_part + r];
#pragma unroll
                for (int i = 0; i < 4; ++i) fold(v[i]);
            }
            for (; p < n_parts; p += 8) fold(part[(size_t)p * ld_part + r]);
        }
#pragma unroll
        for (int off = 4; off >= 1; off >>= 1) {
            const float m2 = __shfl_xor(m, off);
            const double s2 = __shfl_xor(sm, off);
            const float mm = fmaxf(m, m2);
            sm = sm * (double)expf(m - mm) + s2 * (double)expf(m2 - mm);
            m = mm;
        }
    }
    const int w = live ? target[r] : -1;
    const WlWord wd = wl_lookup(segs, w, true);             // (a row that is not live asks for word -1, which no segment holds)
    const int K4 = wd.K4, toff = wd.toff;
    const f32x4 *brow = wd.brow;
    float acc = 0.0f;
    if (brow) {
        const f32x4 *trow = reinterpret_cast<const f32x4 *>(T + (size_t)r * ldt + toff);
        // the lane's whole share of both rows is requested before any of it is used (k <= 256: at most 8 x 16 B each, as
        // wl_dot does for the weight row): one memory round trip per row instead of one per 32 k-values
        f32x4 bv[8], tv[8];
#pragma unroll
        for (int c8 = 0; c8 < 8; ++c8) {
            const int kc = sub + 8 * c8;
            const bool in = kc < K4;
            bv[c8] = in ? brow[kc] : f32x4{0.f, 0.f, 0.f, 0.f};
            tv[c8] = in ? trow[kc] : f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int c8 = 0; c8 < 8; ++c8) {
            if (sub + 8 * c8 >= K4) continue;
            acc = fmaf(bv[c8][0], tv[c8][0], acc);
            acc = fmaf(bv[c8][1], tv[c8][1], acc);
            acc = fmaf(bv[c8][2], tv[c8][2], acc);
            acc = fmaf(bv[c8][3], tv[c8][3], acc);
        }
        for (int kc = sub + 64; kc < K4; kc += 8) {             // k > 256 (untied models): the tail, as wl_dot
            const f32x4 b = brow[kc], t = trow[kc];
            acc = fmaf(b[0], t[0], acc);
            acc = fmaf(b[1], t[1], acc);
            acc = fmaf(b[2], t[2], acc);
            acc = fmaf(b[3], t[3], acc);
        }
    }
    acc = wl_sum8(acc);
    if (!live || sub != 0) return;
    double nll;
    if (!brow) {                       // a target outside every segment (the host checks ids before the launch)
        if (flags) atomicOr(flags, 2);
        nll = __longlong_as_double(0x7ff8000000000000LL);
    } else {
        const float y = acc + b2[w];
        double l = 0.0;
        if (!SELF_NORM) {
            l = (double)m + log(sm);
            if (!(fabs(l) < 1.0e300) && flags) atomicOr(flags, 1);      // as beam_step_kernel: inf / nan from the fixed-reference form
        }
        nll = l - (double)y;
    }
    nll_seq[r] += nll;
    if (nll_tok) nll_tok[r] = nll;
}

// (called by jlm_score_frames, jlm_decode.hip; exported for the tests) target, nll_tok: the step's row of the [n_steps][n_rows] arrays
extern "C" int jlm_score_fold(const jlm_segment *segs_host, int n_segs, const float *b2, const float *T, int ldt, const float *part, int ld_part,
                   int n_parts, int self_norm, const int *target, const int *n_dev, int n_rows_max, double *nll_seq, double *nll_tok,
                   int *flags, void *stream) {
    if (n_segs < 1 || n_segs > JLM_MAX_SEGMENTS || ldt % 4 != 0) return -1;
    if (n_rows_max <= 0) return 0;
    SegTable t;
    t.n = n_segs;
    for (int i = 0; i < n_segs; ++i) {
        if (segs_host[i].k % 4 != 0 || segs_host[i].ldb % 4 != 0 || segs_host[i].t_off % 4 != 0) return -1;
        t.s[i] = segs_host[i];
    }
    const dim3 grid((n_rows_max + SF_ROWS - 1) / SF_ROWS);
    const float2 *pp = reinterpret_cast<const float2 *>(part);
    if (self_norm)
        hipLaunchKernelGGL(score_fold_kernel<1>, grid, dim3(SF_THREADS), 0, (hipStream_t)stream, t, b2, T, ldt, pp, ld_part, 0, target,
                           n_dev, n_rows_max, nll_seq, nll_tok, flags);
    else
        hipLaunchKernelGGL(score_fold_kernel<0>, grid, dim3(SF_THREADS), 0, (hipStream_t)stream, t, b2, T, ldt, pp, ld_part, n_parts,
                           target, n_dev, n_rows_max, nll_seq, nll_tok, flags);
    JLM_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// sample_rows_kernel -- one ancestral-sampling draw per live row of materialised f32 logits y[r, 0:n_cols] (jlm_sample_rows,
// include/jlm_hip.h; the last kernel of a jlm_generate_frames frame).  What the reference's sample(pred, temperature) does on the host
// (decoder/model.py:28-33, 213-245), as an inverse CDF in word-id order with counter-based random numbers.
//
// One workgroup of SR_WAVES waves per row.  The row is read as 16-byte chunks (4 words): an "iteration" is 64 consecutive chunks, one
// per lane (coalesced, 1 KB per wave load), and wave w owns the contiguous iterations [w * ipw, (w + 1) * ipw) -- wave spans in word
// order.  Three passes over a row:
//   1  max m (and the lowest id attaining it: the greedy draw), every wave over its span, merged in wave order.
//   2  per iteration, each lane's chunk mass ((e0 + e1) + e2) + e3 (e = expf((y - m) / tau) in f32, summed in f64), an inclusive
//      Hillis-Steele scan of those over the 64 lanes, and the wave total W_w += the scan's last lane; beside it the tau = 1 sum
//      S1 = sum expf(y - m) (lane-sequential, xor-tree over the wave) for the nll.  S = ((W_0 + W_1) + W_2) + W_3.
//   3  t = u S; the wave w whose prefix first exceeds t re-reads its span ALONE, recomputing pass 2's chunk masses and scans in the
//      same order (bit-identical W_w chain), and stops in the iteration where acc + total > t - P_w: the first lane whose
//      acc + scan > t - P_w, then the first word of that lane's chunk whose running sum crosses.  Where rounding leaves no crossing
//      (t - P_w rounded up, or a lane's own sum short of its scan value by an ulp) the draw is the last word with non-zero mass
//      before that point.
// The summation order is a fixed function of n_cols and the launch shape: the same row gives the same draw on every run.
#define SR_WAVES 4
#define SR_THREADS (64 * SR_WAVES)
#define SR_UNROLL 4

__device__ __forceinline__ double sr_uniform(unsigned long long seed, int step, int row) {
    unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (((unsigned long long)(unsigned)step << 32) | ((unsigned long long)(unsigned)row + 1ull));
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return ((double)(z >> 11) + 0.5) * 0x1.0p-53;
}

// chunk c's words; words past n_cols read as -inf (the row's padding is never trusted)
__device__ __forceinline__ f32x4 sr_load(const f32x4 *row, int c, int n4, int n_cols) {
    f32x4 v = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    if (c < n4) {
        v = row[c];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (4 * c + j >= n_cols) v[j] = -INFINITY;
    }
    return v;
}

// the tempered masses of a chunk (pass 2 and pass 3 call this same code, so both see the same bits)
__device__ __forceinline__ f32x4 sr_mass(const f32x4 v, float m, float inv_tau) {
    f32x4 e;
#pragma unroll
    for (int j = 0; j < 4; ++j) e[j] = expf((v[j] - m) * inv_tau);
    return e;
}

__device__ __forceinline__ double sr_chunk_sum(const f32x4 e) {
    double c = (double)e[0];
    c += (double)e[1];
    c += (double)e[2];
    c += (double)e[3];
    return c;
}

__device__ __forceinline__ double sr_scan(double c, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double t = __shfl_up(c, off);
        if (lane >= off) c += t;
    }
    return c;
}

template <int SELF_NORM>
__global__ __launch_bounds__(SR_THREADS) void sample_rows_kernel(
    const float *__restrict__ y, int ld, int n_cols, const int *__restrict__ n_dev, int n_rows_max, int greedy, float inv_tau,
    unsigned long long seed, int step, const int *__restrict__ row_id, const int *__restrict__ forced, int *__restrict__ done,
    int stop_id, int *__restrict__ word, int *__restrict__ ids, double *__restrict__ nll, int *flags) {
    const int r = blockIdx.x;
    const int n = n_dev ? min(*n_dev, n_rows_max) : n_rows_max;
    if (r >= n) return;                                   // uniform over the workgroup: no barrier is skipped by part of it
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (forced && forced[r] >= 0) {                       // a forced (prompt) position: its word passes through
        if (tid == 0) { word[r] = forced[r]; ids[r] = -1; nll[r] = 0.0; }
        return;
    }
    if (done && done[r]) {                                // a row that has drawn its stop word: masked (its word stays valid)
        if (tid == 0) { ids[r] = -1; nll[r] = 0.0; }
        return;
    }
    const f32x4 *row = reinterpret_cast<const f32x4 *>(y + (size_t)r * ld);
    const int n4 = (n_cols + 3) >> 2, n_it = (n4 + 63) >> 6;
    const int ipw = (n_it + SR_WAVES - 1) / SR_WAVES;
    const int it0 = wv * ipw, it1 = min(it0 + ipw, n_it);
    __shared__ float s_m[SR_WAVES];
    __shared__ int s_i[SR_WAVES];
    __shared__ double s_w[SR_WAVES], s_s1[SR_WAVES];

    // ---- pass 1: max, lowest id attaining it
    float m = -INFINITY;
    int mi = 0x7fffffff;
    for (int it = it0; it < it1; it += SR_UNROLL) {
        f32x4 v[SR_UNROLL];
#pragma unroll
        for (int k = 0; k < SR_UNROLL; ++k) v[k] = it + k < it1 ? sr_load(row, (it + k) * 64 + lane, n4, n_cols) : f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
        for (int k = 0; k < SR_UNROLL; ++k)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (v[k][j] > m) { m = v[k][j]; mi = 4 * ((it + k) * 64 + lane) + j; }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float m2 = __shfl_xor(m, off);
        const int i2 = __shfl_xor(mi, off);
        if (m2 > m || (m2 == m && i2 < mi)) { m = m2; mi = i2; }
    }
    if (lane == 0) { s_m[wv] = m; s_i[wv] = mi; }
    __syncthreads();
    m = s_m[0];
    mi = s_i[0];
    for (int w = 1; w < SR_WAVES; ++w)
        if (s_m[w] > m) { m = s_m[w]; mi = s_i[w]; }      // waves in word order: a tie keeps the earlier wave's (lower) id

    // ---- pass 2: the tempered chunk masses' scans (wave totals) and the tau = 1 sum
    const bool fin_m = m > -INFINITY && m < INFINITY;
    const bool same = inv_tau == 1.0f;
    double W = 0.0, s1 = 0.0;
    if (fin_m && !(greedy && SELF_NORM)) {
        for (int it = it0; it < it1; it += SR_UNROLL) {
            f32x4 v[SR_UNROLL];
#pragma unroll
            for (int k = 0; k < SR_UNROLL; ++k) v[k] = it + k < it1 ? sr_load(row, (it + k) * 64 + lane, n4, n_cols) : f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
            for (int k = 0; k < SR_UNROLL; ++k) {
                if (it + k >= it1) break;                 // wave-uniform
                const f32x4 e1 = sr_mass(v[k], m, 1.0f);
                if (!SELF_NORM) {
                    s1 += (double)e1[0];
                    s1 += (double)e1[1];
                    s1 += (double)e1[2];
                    s1 += (double)e1[3];
                }
                if (!greedy) {
                    const f32x4 e = same ? e1 : sr_mass(v[k], m, inv_tau);
                    const double s = sr_scan(sr_chunk_sum(e), lane);
                    W += __shfl(s, 63);
                }
            }
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s1 += __shfl_xor(s1, off);
    if (lane == 0) { s_w[wv] = W; s_s1[wv] = s1; }
    __syncthreads();
    double S = 0.0, S1 = 0.0;
    for (int w = 0; w < SR_WAVES; ++w) { S += s_w[w]; S1 += s_s1[w]; }
    const bool ok = fin_m && (greedy || (S > 0.0 && S < INFINITY)) && (SELF_NORM || (S1 > 0.0 && S1 < INFINITY));
    if (!ok) {                                            // a NaN / inf logit: flagged; the row's next word stays a valid id
        if (tid == 0) {
            if (flags) atomicOr(flags, 1);
            ids[r] = -1;
            nll[r] = __longlong_as_double(0x7ff8000000000000LL);
            word[r] = 0;
            if (done) done[r] = 1;
        }
        return;
    }

    // ---- pass 3: the crossing
    int pick = mi, writer = 0;
    if (!greedy) {
        const double t = sr_uniform(seed, step, row_id ? row_id[r] : r) * S;
        int ws = -1;
        double tp = INFINITY, P = 0.0;
        for (int w = 0; w < SR_WAVES; ++w) {
            const double Pn = P + s_w[w];
            if (Pn > t) { ws = w; tp = t - P; break; }
            P = Pn;
        }
        if (ws < 0)                                       // u S rounded up to S: the last word with mass, i.e. of the last such wave
            for (int w = 0; w < SR_WAVES; ++w)
                if (s_w[w] > 0.0) ws = w;
        if (wv != ws) return;
        writer = ws * 64;
        double acc = 0.0;
        int last = -1;                                    // the lane's last word with non-zero mass so far
        pick = -1;
        bool crossed = false;
        for (int it = it0; it < it1 && !crossed; it += SR_UNROLL) {
            f32x4 v[SR_UNROLL];
#pragma unroll
            for (int k = 0; k < SR_UNROLL; ++k) v[k] = it + k < it1 ? sr_load(row, (it + k) * 64 + lane, n4, n_cols) : f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
            for (int k = 0; k < SR_UNROLL; ++k) {
                if (it + k >= it1) break;
                const int c = (it + k) * 64 + lane;
                const f32x4 e = same ? sr_mass(v[k], m, 1.0f) : sr_mass(v[k], m, inv_tau);
                const double s = sr_scan(sr_chunk_sum(e), lane);
                const double total = __shfl(s, 63);
                int lnz = -1;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (e[j] > 0.0f) lnz = 4 * c + j;
                if (acc + total > tp) {
                    const unsigned long long b = __ballot(acc + s > tp);     // lane 63 at least: its scan value is `total`
                    const int l = __ffsll(b) - 1;
                    const double prev = __shfl_up(s, 1);
                    int cand = -1;
                    if (lane == l) {
                        double cum = lane == 0 ? 0.0 : prev;
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            cum += (double)e[j];
                            if (cand < 0 && acc + cum > tp) cand = 4 * c + j;
                        }
                        if (cand < 0) cand = lnz;
                    }
                    int val = lane < l ? lnz : (lane == l ? cand : -1);
                    val = max(val, last);
#pragma unroll
                    for (int off = 32; off >= 1; off >>= 1) val = max(val, __shfl_xor(val, off));
                    pick = val;
                    crossed = true;
                    break;
                }
                acc += total;
                if (lnz >= 0) last = lnz;
            }
        }
        if (!crossed) {                                   // rounding left no crossing in the span: its last word with mass
            int val = last;
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) val = max(val, __shfl_xor(val, off));
            pick = val;
        }
        if (pick < 0 || pick >= n_cols) pick = mi;       // (unreachable: wave ws holds mass)
    }
    if (tid != writer) return;
    const float yv = y[(size_t)r * ld + pick];
    ids[r] = pick;
    word[r] = pick;
    nll[r] = SELF_NORM ? -(double)yv : ((double)m + log(S1)) - (double)yv;
    if (done && pick == stop_id) done[r] = 1;
}

extern "C" int jlm_sample_rows(const float *y, int ld_y, int n_cols, int n_rows_max, const int *n_dev, double temperature,
                               uint64_t seed, int step, const int *row_id, const int *forced, int *done, int stop_id, int self_norm,
                               int *word, int *ids, double *nll, int *flags, void *stream) {
    if (n_cols < 1 || ld_y % 4 != 0 || ld_y < ((n_cols + 3) & ~3) || ((uintptr_t)y & 15) != 0) return -1;
    if (!(temperature >= 0.0 && temperature < INFINITY) || !word || !ids || !nll) return -1;
    if (n_rows_max <= 0) return 0;
    const int greedy = temperature == 0.0;
    const float inv_tau = greedy ? 1.0f : (float)(1.0 / temperature);
    if (!greedy && !(inv_tau > 0.0f && inv_tau < INFINITY)) return -1;
    const dim3 grid(n_rows_max);
    if (self_norm)
        hipLaunchKernelGGL(sample_rows_kernel<1>, grid, dim3(SR_THREADS), 0, (hipStream_t)stream, y, ld_y, n_cols, n_dev, n_rows_max,
                           greedy, inv_tau, (unsigned long long)seed, step, row_id, forced, done, stop_id, word, ids, nll, flags);
    else
        hipLaunchKernelGGL(sample_rows_kernel<0>, grid, dim3(SR_THREADS), 0, (hipStream_t)stream, y, ld_y, n_cols, n_dev, n_rows_max,
                           greedy, inv_tau, (unsigned long long)seed, step, row_id, forced, done, stop_id, word, ids, nll, flags);
    JLM_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// sample_rows_trunc_kernel -- sample_rows_kernel's draw over a truncated distribution: top-k, then nucleus (top-p) on what top-k
// kept (jlm_sample_rows_trunc, include/jlm_hip.h; the last kernel of a jlm_generate_frames_trunc frame).
//
// Words are ranked by (logit descending, id ascending), so every kept set is a threshold cut {j : (y_j, -j) >= (y*, -id*)}.  The kernel
// finds (y*, id*) by a radix selection on the order-preserving u32 image of the f32 logit (tr_key) and then runs sample_rows_kernel's
// passes 2 and 3 with the mass of every word outside the cut set to zero: same layout, same summation order, same u.
//
// Selection.  The key's 32 bits are taken as three digits of 11 / 11 / 10 bits, most significant first.  A level reads the row once
// and builds, over the words that match the digits chosen so far, a histogram in LDS: a u32 count per bin, and for top-p the bin's
// mass as a u64 fixed-point sum (round(expf(.) * 2^s), s chosen by the host so that n_cols masses cannot overflow).  Both are integer
// LDS atomics: the sums are exact, so the order in which the lanes arrive cannot change them.  A workgroup scan over the bins,
// highest first, finds the bin where the running count reaches k (top-k) or the running mass reaches ceil(p * mass(K)) (top-p,
// restricted to the words top-k kept); the next level descends into it.  After the third level the bin is one exact logit value: the
// number of words to take at that value is the remainder, and when it is fewer than the words holding that value a last pass finds
// the id of the remainder-th of them in id order (tr_tie_id).  Top-k's first level is counted during pass 1.
//
// Passes over a row: 1 (max) + 2 (top-k levels two and three) + 3 (top-p) + 1.25 (the draw's passes 2 and 3), and 1.25 for each cut
// that splits equal logits: at most 9.75, whatever k, p and n_cols are.  top_k = 1 needs no selection (the cut is pass 1's argmax).
#define TR_BINS 2048
#define TR_PER (TR_BINS / SR_THREADS)
#define TR_ALL_IDS 0x7fffffff

// the order-preserving u32 image of a logit (-0 ranks with +0, as it compares)
__device__ __forceinline__ unsigned tr_key(float v) {
    const unsigned b = __float_as_uint(v == 0.0f ? 0.0f : v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// a cut in rank order: the words at or above (key, id)
struct TrCut {
    unsigned key;
    int id;
    __device__ __forceinline__ bool keeps(unsigned k, int i) const { return k > key || (k == key && i <= id); }
};

struct TrFound {
    unsigned bin, above_cnt, bin_cnt;                    // the crossing bin, the count above it and in it
    unsigned long long above_mass, bin_mass, target;     // the masses likewise; the mass target the search used
};

struct TrShared {
    unsigned cnt[TR_BINS];
    unsigned long long mass[TR_BINS];
    unsigned wave_cnt[SR_WAVES];
    unsigned long long wave_mass[SR_WAVES];
    TrFound found;
    int tie_id;
};

__device__ __forceinline__ unsigned long long tr_fix(float e, double fix) { return (unsigned long long)((double)e * fix + 0.5); }

// One selection level: the histogram of digit `level` over the words of `within` whose higher digits equal `prefix`.
template <bool MASS>
__device__ __forceinline__ void tr_hist(const f32x4 *row, int n4, int n_cols, int tid, int level, unsigned prefix, const TrCut within,
                                        float m, float inv_tau, double fix, TrShared &sh) {
    const int hs = level == 1 ? 21 : 10, ls = level == 0 ? 21 : (level == 1 ? 10 : 0);
    const unsigned mask = level == 2 ? 0x3ffu : 0x7ffu;
    for (int c0 = tid; c0 < n4; c0 += SR_THREADS * SR_UNROLL) {
        f32x4 v[SR_UNROLL];
#pragma unroll
        for (int k = 0; k < SR_UNROLL; ++k) v[k] = sr_load(row, c0 + k * SR_THREADS, n4, n_cols);
#pragma unroll
        for (int k = 0; k < SR_UNROLL; ++k) {
            const int c = c0 + k * SR_THREADS;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int id = 4 * c + j;
                const unsigned key = tr_key(v[k][j]);
                if (id >= n_cols || (level && (key >> hs) != prefix) || !within.keeps(key, id)) continue;
                const unsigned bin = (key >> ls) & mask;
                atomicAdd(&sh.cnt[bin], 1u);
                if (MASS) atomicAdd(&sh.mass[bin], tr_fix(expf((v[k][j] - m) * inv_tau), fix));
            }
        }
    }
}

// The bin, highest first, where the running count (MASS: mass) reaches `target` (MASS with p > 0: ceil(p * the histogram's total),
// at least 1).  Thread t scans bins TR_BINS - 1 - TR_PER t downwards and clears them for the next level.  No crossing (target above
// the total): bin 0 with zero counts.
template <bool MASS>
__device__ __forceinline__ TrFound tr_find(unsigned long long target, double p, int tid, TrShared &sh) {
    __syncthreads();                                      // the histogram is complete
    const int lane = tid & 63, wv = tid >> 6;
    unsigned c[TR_PER], lc = 0;
    unsigned long long w[TR_PER], lm = 0;
#pragma unroll
    for (int i = 0; i < TR_PER; ++i) {
        const int b = TR_BINS - 1 - (tid * TR_PER + i);
        c[i] = sh.cnt[b];
        sh.cnt[b] = 0;
        lc += c[i];
        w[i] = 0;
        if (MASS) {
            w[i] = sh.mass[b];
            sh.mass[b] = 0;
            lm += w[i];
        }
    }
    unsigned ic = lc;
    unsigned long long im = lm;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned tc = __shfl_up(ic, off);
        const unsigned long long tm = __shfl_up(im, off);
        if (lane >= off) { ic += tc; im += tm; }
    }
    if (lane == 63) { sh.wave_cnt[wv] = ic; sh.wave_mass[wv] = im; }
    if (tid == 0) sh.found = TrFound{0u, 0u, 0u, 0ull, 0ull, 0ull};
    __syncthreads();
    unsigned long long total = 0;
    for (int x = 0; x < SR_WAVES; ++x) {
        if (x < wv) { ic += sh.wave_cnt[x]; im += sh.wave_mass[x]; }
        total += sh.wave_mass[x];
    }
    if (MASS && p > 0.0) {
        const double t = ceil(p * (double)total);
        target = t >= (double)total ? total : (unsigned long long)t;
        if (target < 1) target = 1;
    }
    const unsigned long long inc = MASS ? im : (unsigned long long)ic, loc = MASS ? lm : (unsigned long long)lc;
    if (inc - loc < target && target <= inc) {            // one thread at most: the running sum is monotone
        unsigned long long a = inc - loc, am = im - lm;
        unsigned ac = ic - lc;
        bool hit = false;
#pragma unroll
        for (int i = 0; i < TR_PER; ++i) {
            const unsigned long long x = MASS ? w[i] : (unsigned long long)c[i];
            if (!hit && a + x >= target) {
                sh.found = TrFound{(unsigned)(TR_BINS - 1 - (tid * TR_PER + i)), ac, c[i], am, w[i], 0ull};
                hit = true;
            }
            a += x;
            ac += c[i];
            am += w[i];
        }
    }
    __syncthreads();
    TrFound f = sh.found;
    f.target = target;
    return f;
}

// the id of the t-th word (t >= 1), in id order, whose key is `key`; TR_ALL_IDS when there are fewer.  Wave spans in word order as
// in the draw: every wave counts its span, then the wave that holds the t-th walks its span again.
__device__ __forceinline__ int tr_tie_id(const f32x4 *row, int n4, int n_cols, int it0, int it1, int tid, unsigned key, unsigned t,
                                         TrShared &sh) {
    const int lane = tid & 63, wv = tid >> 6;
    auto count = [&](const f32x4 v, int c) {
        unsigned n = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) n += 4 * c + j < n_cols && tr_key(v[j]) == key;
        return n;
    };
    unsigned n = 0;
    for (int it = it0; it < it1; ++it) n += count(sr_load(row, it * 64 + lane, n4, n_cols), it * 64 + lane);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) n += __shfl_xor(n, off);
    __syncthreads();                                      // wave_cnt and tie_id are free (tr_find's readers are past it)
    if (lane == 0) sh.wave_cnt[wv] = n;
    if (tid == 0) sh.tie_id = TR_ALL_IDS;
    __syncthreads();
    int ws = -1;
    unsigned before = 0;
    for (int x = 0; x < SR_WAVES; ++x) {
        if (before + sh.wave_cnt[x] >= t) { ws = x; break; }
        before += sh.wave_cnt[x];
    }
    if (wv == ws) {
        unsigned acc = before;
        for (int it = it0; it < it1; ++it) {
            const int c = it * 64 + lane;
            const f32x4 v = sr_load(row, c, n4, n_cols);
            const unsigned mine = count(v, c);
            unsigned s = mine;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const unsigned x = __shfl_up(s, off);
                if (lane >= off) s += x;
            }
            const unsigned total = __shfl(s, 63);
            if (acc + total >= t) {                       // wave-uniform
                const int l = __ffsll(__ballot(acc + s >= t)) - 1;
                if (lane == l) {
                    unsigned need = t - (acc + s - mine);
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (need && 4 * c + j < n_cols && tr_key(v[j]) == key && --need == 0) sh.tie_id = 4 * c + j;
                }
                break;
            }
            acc += total;
        }
    }
    __syncthreads();
    return sh.tie_id;
}

// the masses of chunk c with every word outside the cut at zero
__device__ __forceinline__ f32x4 tr_keep(f32x4 e, const f32x4 v, int c, const TrCut cut) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (!cut.keeps(tr_key(v[j]), 4 * c + j)) e[j] = 0.0f;
    return e;
}

template <int SELF_NORM>
__global__ __launch_bounds__(SR_THREADS) void sample_rows_trunc_kernel(
    const float *__restrict__ y, int ld, int n_cols, const int *__restrict__ n_dev, int n_rows_max, float inv_tau, int top_k,
    double top_p, double fix, unsigned long long seed, int step, const int *__restrict__ row_id, const int *__restrict__ forced,
    int *__restrict__ done, int stop_id, int *__restrict__ word, int *__restrict__ ids, double *__restrict__ nll, int *flags) {
    const int r = blockIdx.x;
    const int n = n_dev ? min(*n_dev, n_rows_max) : n_rows_max;
    if (r >= n) return;                                   // uniform over the workgroup, as every exit before the last barrier
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (forced && forced[r] >= 0) {
        if (tid == 0) { word[r] = forced[r]; ids[r] = -1; nll[r] = 0.0; }
        return;
    }
    if (done && done[r]) {
        if (tid == 0) { ids[r] = -1; nll[r] = 0.0; }
        return;
    }
    const f32x4 *row = reinterpret_cast<const f32x4 *>(y + (size_t)r * ld);
    const int n4 = (n_cols + 3) >> 2, n_it = (n4 + 63) >> 6;
    const int ipw = (n_it + SR_WAVES - 1) / SR_WAVES;
    const int it0 = wv * ipw, it1 = min(it0 + ipw, n_it);
    __shared__ TrShared sh;
    __shared__ float s_m[SR_WAVES];
    __shared__ int s_i[SR_WAVES], s_bad[SR_WAVES];
    __shared__ double s_w[SR_WAVES], s_s1[SR_WAVES];
    const bool k_on = top_k > 1, p_on = top_p > 0.0 && top_k != 1;
    for (int b = tid; b < TR_BINS; b += SR_THREADS) { sh.cnt[b] = 0; sh.mass[b] = 0; }
    __syncthreads();

    // ---- pass 1: max, lowest id attaining it; a NaN anywhere; top-k's first-level counts
    float m = -INFINITY;
    int mi = 0x7fffffff;
    bool bad = false;
    for (int it = it0; it < it1; it += SR_UNROLL) {
        f32x4 v[SR_UNROLL];
#pragma unroll
        for (int k = 0; k < SR_UNROLL; ++k) v[k] = it + k < it1 ? sr_load(row, (it + k) * 64 + lane, n4, n_cols) : f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
        for (int k = 0; k < SR_UNROLL; ++k)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int id = 4 * ((it + k) * 64 + lane) + j;
                if (v[k][j] > m) { m = v[k][j]; mi = id; }
                bad |= v[k][j] != v[k][j];
                if (k_on && it + k < it1 && id < n_cols) atomicAdd(&sh.cnt[tr_key(v[k][j]) >> 21], 1u);
            }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float m2 = __shfl_xor(m, off);
        const int i2 = __shfl_xor(mi, off);
        if (m2 > m || (m2 == m && i2 < mi)) { m = m2; mi = i2; }
    }
    const bool wave_bad = __ballot(bad) != 0ull;
    if (lane == 0) { s_m[wv] = m; s_i[wv] = mi; s_bad[wv] = wave_bad; }
    __syncthreads();
    m = s_m[0];
    mi = s_i[0];
    bad = s_bad[0];
    for (int w = 1; w < SR_WAVES; ++w) {
        if (s_m[w] > m) { m = s_m[w]; mi = s_i[w]; }      // waves in word order: a tie keeps the earlier wave's (lower) id
        bad |= s_bad[w] != 0;
    }
    auto flag_row = [&]() {                               // a NaN / inf logit: flagged; the row's next word stays a valid id
        if (tid == 0) {
            if (flags) atomicOr(flags, 1);
            ids[r] = -1;
            nll[r] = __longlong_as_double(0x7ff8000000000000LL);
            word[r] = 0;
            if (done) done[r] = 1;
        }
    };
    if (bad || !(m > -INFINITY && m < INFINITY)) { flag_row(); return; }

    // ---- the cut: top-k by counts, then top-p by masses within it
    TrCut cut{0u, TR_ALL_IDS};                            // keeps every word
    if (top_k == 1) cut = TrCut{tr_key(m), mi};
    if (k_on) {
        unsigned rem = (unsigned)top_k, prefix = 0;
        TrFound f{};
        for (int level = 0; level < 3; ++level) {
            if (level) tr_hist<false>(row, n4, n_cols, tid, level, prefix, cut, m, inv_tau, fix, sh);
            f = tr_find<false>(rem, 0.0, tid, sh);
            rem -= f.above_cnt;
            prefix = (prefix << (level == 2 ? 10 : 11)) | f.bin;
        }
        const int id = rem < f.bin_cnt ? tr_tie_id(row, n4, n_cols, it0, it1, tid, prefix, rem, sh) : TR_ALL_IDS;
        cut = TrCut{prefix, id};
    }
    if (p_on) {
        const TrCut K = cut;
        unsigned long long rem = 0;
        unsigned prefix = 0;
        TrFound f{};
        for (int level = 0; level < 3; ++level) {
            tr_hist<true>(row, n4, n_cols, tid, level, prefix, K, m, inv_tau, fix, sh);
            f = tr_find<true>(rem, level ? 0.0 : top_p, tid, sh);
            if (level == 0) rem = f.target;
            rem -= f.above_mass;
            prefix = (prefix << (level == 2 ? 10 : 11)) | f.bin;
        }
        // the bin is one logit value: bin_cnt words of one mass each, taken in id order until the target is reached
        const unsigned cnt = max(f.bin_cnt, 1u);
        const unsigned long long one = max(f.bin_mass / cnt, 1ull);
        const unsigned long long t = min(max((rem + one - 1) / one, 1ull), (unsigned long long)cnt);
        int id = prefix == K.key ? K.id : TR_ALL_IDS;
        if (t < cnt) id = tr_tie_id(row, n4, n_cols, it0, it1, tid, prefix, (unsigned)t, sh);
        cut = TrCut{prefix, id};
    }

    // ---- pass 2 (sample_rows_kernel's, over the kept words): the tempered chunk masses' scans (wave totals) and the tau = 1 sum
    const bool same = inv_tau == 1.0f;
    double W = 0.0, s1 = 0.0;
    for (int it = it0; it < it1; it += SR_UNROLL) {
        f32x4 v[SR_UNROLL];
#pragma unroll
        for (int k = 0; k < SR_UNROLL; ++k) v[k] = it + k < it1 ? sr_load(row, (it + k) * 64 + lane, n4, n_cols) : f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
        for (int k = 0; k < SR_UNROLL; ++k) {
            if (it + k >= it1) break;                     // wave-uniform
            const f32x4 e1 = sr_mass(v[k], m, 1.0f);
            if (!SELF_NORM) {
                s1 += (double)e1[0];
                s1 += (double)e1[1];
                s1 += (double)e1[2];
                s1 += (double)e1[3];
            }
            const f32x4 e = tr_keep(same ? e1 : sr_mass(v[k], m, inv_tau), v[k], (it + k) * 64 + lane, cut);
            const double s = sr_scan(sr_chunk_sum(e), lane);
            W += __shfl(s, 63);
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s1 += __shfl_xor(s1, off);
    if (lane == 0) { s_w[wv] = W; s_s1[wv] = s1; }
    __syncthreads();
    double S = 0.0, S1 = 0.0;
    for (int w = 0; w < SR_WAVES; ++w) { S += s_w[w]; S1 += s_s1[w]; }
    if (!(S > 0.0 && S < INFINITY && (SELF_NORM || (S1 > 0.0 && S1 < INFINITY)))) { flag_row(); return; }

    // ---- pass 3 (sample_rows_kernel's, over the kept words): the crossing
    const double t = sr_uniform(seed, step, row_id ? row_id[r] : r) * S;
    int ws = -1;
    double tp = INFINITY, P = 0.0;
    for (int w = 0; w < SR_WAVES; ++w) {
        const double Pn = P + s_w[w];
        if (Pn > t) { ws = w; tp = t - P; break; }
        P = Pn;
    }
    if (ws < 0)                                           // u S rounded up to S: the last kept word with mass
        for (int w = 0; w < SR_WAVES; ++w)
            if (s_w[w] > 0.0) ws = w;
    if (wv != ws) return;
    double acc = 0.0;
    int last = -1, pick = -1;                             // last: the lane's last kept word with non-zero mass so far
    bool crossed = false;
    for (int it = it0; it < it1 && !crossed; it += SR_UNROLL) {
        f32x4 v[SR_UNROLL];
#pragma unroll
        for (int k = 0; k < SR_UNROLL; ++k) v[k] = it + k < it1 ? sr_load(row, (it + k) * 64 + lane, n4, n_cols) : f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
        for (int k = 0; k < SR_UNROLL; ++k) {
            if (it + k >= it1) break;
            const int c = (it + k) * 64 + lane;
            const f32x4 e = tr_keep(same ? sr_mass(v[k], m, 1.0f) : sr_mass(v[k], m, inv_tau), v[k], c, cut);
            const double s = sr_scan(sr_chunk_sum(e), lane);
            const double total = __shfl(s, 63);
            int lnz = -1;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (e[j] > 0.0f) lnz = 4 * c + j;
            if (acc + total > tp) {
                const unsigned long long b = __ballot(acc + s > tp);         // lane 63 at least: its scan value is `total`
                const int l = __ffsll(b) - 1;
                const double prev = __shfl_up(s, 1);
                int cand = -1;
                if (lane == l) {
                    double cum = lane == 0 ? 0.0 : prev;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        cum += (double)e[j];
                        if (cand < 0 && e[j] > 0.0f && acc + cum > tp) cand = 4 * c + j;
                    }
                    if (cand < 0) cand = lnz;
                }
                int val = lane < l ? lnz : (lane == l ? cand : -1);
                val = max(val, last);
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) val = max(val, __shfl_xor(val, off));
                pick = val;
                crossed = true;
                break;
            }
            acc += total;
            if (lnz >= 0) last = lnz;
        }
    }
    if (!crossed) {                                       // rounding left no crossing in the span: its last kept word with mass
        int val = last;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) val = max(val, __shfl_xor(val, off));
        pick = val;
    }
    if (pick < 0 || pick >= n_cols) pick = mi;            // (unreachable: wave ws holds kept mass; mi is always kept)
    if (tid != ws * 64) return;
    const float yv = y[(size_t)r * ld + pick];
    ids[r] = pick;
    word[r] = pick;
    nll[r] = SELF_NORM ? -(double)yv : ((double)m + log(S1)) - (double)yv;
    if (done && pick == stop_id) done[r] = 1;
}

extern "C" int jlm_sample_rows_trunc(const float *y, int ld_y, int n_cols, int n_rows_max, const int *n_dev, double temperature,
                                     uint64_t seed, int step, const int *row_id, const int *forced, int *done, int stop_id,
                                     int self_norm, int top_k, double top_p, int *word, int *ids, double *nll, int *flags,
                                     void *stream) {
    if (!(top_p > 0.0)) return -1;                        // NaN included
    if (top_k <= 0 || top_k >= n_cols) top_k = 0;
    if (top_p >= 1.0) top_p = 0.0;
    if (temperature == 0.0 || (top_k == 0 && top_p == 0.0))     // greedy, or nothing to cut: the untruncated draw
        return jlm_sample_rows(y, ld_y, n_cols, n_rows_max, n_dev, temperature, seed, step, row_id, forced, done, stop_id, self_norm,
                               word, ids, nll, flags, stream);
    if (n_cols < 1 || ld_y % 4 != 0 || ld_y < ((n_cols + 3) & ~3) || ((uintptr_t)y & 15) != 0) return -1;
    if (!(temperature > 0.0 && temperature < INFINITY) || !word || !ids || !nll) return -1;
    if (n_rows_max <= 0) return 0;
    const float inv_tau = (float)(1.0 / temperature);
    if (!(inv_tau > 0.0f && inv_tau < INFINITY)) return -1;
    // the masses' fixed point: n_cols of them, each at most 2^s + 1, stay below 2^63
    int bits = 0;
    while ((1ll << bits) < (long long)n_cols) ++bits;
    const double fix = ldexp(1.0, 62 - bits > 52 ? 52 : 62 - bits);
    const dim3 grid(n_rows_max);
    if (self_norm)
        hipLaunchKernelGGL(sample_rows_trunc_kernel<1>, grid, dim3(SR_THREADS), 0, (hipStream_t)stream, y, ld_y, n_cols, n_dev,
                           n_rows_max, inv_tau, top_k, top_p, fix, (unsigned long long)seed, step, row_id, forced, done, stop_id, word,
                           ids, nll, flags);
    else
        hipLaunchKernelGGL(sample_rows_trunc_kernel<0>, grid, dim3(SR_THREADS), 0, (hipStream_t)stream, y, ld_y, n_cols, n_dev,
                           n_rows_max, inv_tau, top_k, top_p, fix, (unsigned long long)seed, step, row_id, forced, done, stop_id, word,
                           ids, nll, flags);
    JLM_LAUNCH_CHECK();
    return 0;
}
