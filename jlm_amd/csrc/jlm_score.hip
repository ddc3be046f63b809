// jlm_score.hip -- the last kernel of a teacher-forced scoring step (jlm_score_frames, include/jlm_hip.h; jlm_decode.hip enqueues
// the step): per live row, the normaliser's (max, sum exp) slices folded into the log-normaliser, the target word's logit, and
// nll = lse - y accumulated in f64.  What the reference's LSTM_Model.evaluate reads off a materialised softmax one word at a time
// (decoder/model.py:200-206, 15-20, 117-119).
//
// A row is 8 lanes of a wave, 8 rows per wave, 32 per workgroup -- the beam step's fold layout (jlm_beam.hip, fused K6 tail):
//   fold    lane `sub` takes the slices p = sub, sub + 8, ...; three xor-shuffle steps merge the 8 partial (max, sum) pairs.
//           Same order and arithmetic as beam_step_kernel's fold, so a row's log-normaliser is the one the decode uses.
//   logit   lane `sub` takes the 16-byte chunks k4 = sub, sub + 8, ... of the target's weight row and the row of T (all requested
//           before the first is used), fmaf in k order, three xor-shuffle adds, + b2[w]: wordlist_kernel<0>'s f32 arithmetic
//           (jlm_edge_logits).
// Latency-bound and tiny next to the step's three matrix kernels: one slice read per lane and slice row, one weight row per row.
#include "jlm_common.h"

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
    int K4 = 0, toff = 0;
    const f32x4 *brow = nullptr;
    for (int si = 0; si < segs.n; ++si)
        if (w >= segs.s[si].v_start && w < segs.s[si].v_end) {
            K4 = segs.s[si].k >> 2;
            toff = segs.s[si].t_off;
            brow = reinterpret_cast<const f32x4 *>(segs.s[si].B + (size_t)(w - segs.s[si].v_start) * segs.s[si].ldb);
        }
    float acc = 0.0f;
    if (brow) {
        const f32x4 *trow = reinterpret_cast<const f32x4 *>(T + (size_t)r * ldt + toff);
        // the lane's whole share of both rows is requested before any of it is used (k <= 256: at most 8 x 16 B each, as
        // wordlist_kernel does): one memory round trip per row instead of one per 32 k-values
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
        for (int kc = sub + 64; kc < K4; kc += 8) {             // k > 256 (untied models): the tail, as wordlist_kernel
            const f32x4 b = brow[kc], t = trow[kc];
            acc = fmaf(b[0], t[0], acc);
            acc = fmaf(b[1], t[1], acc);
            acc = fmaf(b[2], t[2], acc);
            acc = fmaf(b[3], t[3], acc);
        }
    }
    acc += __shfl_xor(acc, 1);
    acc += __shfl_xor(acc, 2);
    acc += __shfl_xor(acc, 4);
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

// (internal: called by jlm_score_frames, jlm_decode.hip) target, nll_tok: the step's row of the [n_steps][n_rows] arrays
int jlm_score_fold(const jlm_segment *segs_host, int n_segs, const float *b2, const float *T, int ldt, const float *part, int ld_part,
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
