// The word-addressed logit: the ONE definition of the arithmetic behind jlm_edge_logits, shared by every kernel whose logit must equal
// it bit for bit -- wordlist_kernel<0 / 1> (csrc/jlm_beam.hip), tail_predict_kernel (csrc/jlm_tail.hip), alt_head_kernel
// (csrc/jlm_alt.hip) and, for the lookup and the lane sum, score_fold_kernel (csrc/jlm_score.hip).
//
// Eight lanes share a word.  Lane `sub` takes the 16-byte pieces kc = sub, sub + 8, ... of the word's weight row, in order, as one fmaf
// chain over elements 0 .. 3 of every piece; the eight partial dots are summed by an xor butterfly over 1, 2, 4; the caller adds b2[w].
// frame_tail_mx6_kernel (csrc/jlm_frame_tail.hip) forms the same chain on a schedule of its own (LDS-DMA, row groups of four, a DPP
// sum, 64 registers): tests/test_gpu_frame_tail.py pins it to this one.
#pragma once
#include "jlm_common.h"

// where word w's weight row lives: K4 16-byte pieces at brow, against T columns toff ..; a word outside every segment: brow NULL, K4 0
struct WlWord {
    int K4, toff;
    const f32x4 *brow;
};

__device__ __forceinline__ WlWord wl_lookup(const SegTable &segs, int w, bool valid) {
    WlWord p{0, 0, nullptr};
    if (valid) {
        for (int si = 0; si < segs.n; ++si)
            if (w >= segs.s[si].v_start && w < segs.s[si].v_end) {
                p.K4 = segs.s[si].k >> 2;
                p.toff = segs.s[si].t_off;
                p.brow = reinterpret_cast<const f32x4 *>(segs.s[si].B + (size_t)(w - segs.s[si].v_start) * segs.s[si].ldb);
            }
    }
    return p;
}

// the sum over the eight lanes of a word (the same bits on all eight)
__device__ __forceinline__ float wl_sum8(float acc) {
    acc += __shfl_xor(acc, 1);
    acc += __shfl_xor(acc, 2);
    acc += __shfl_xor(acc, 4);
    return acc;
}

// acc[r] = the word's dot with staged row r (rows: ROWS rows of ldt floats in LDS), for the rows with rc + r < nrows -- rc the pass'
// first row, nrows the rows there are -- summed over the eight lanes; acc[r] = 0 for the other rows.  Every lane of the wave calls
// this (the sum is a wave exchange); a lane without a word passes K4 = 0 and reads nothing.
// Two choices keep wordlist_kernel's code close to what it was before the function was shared: the bound is the caller's own
// expression rc + r < nrows (tested as r < nrows - rc the sixteen masks spill 32 scalar registers to lanes), and the staged row is
// read as four floats, which the compiler pairs into 8-byte LDS reads as it did there.  The form with one 16-byte read and the
// other bound, the two together, put three bench.py figures outside the parent's spread; this one none in the run that followed
// (profiles/shared_arith_bench_ab.txt, run 1 against runs 2 and 3).
template <int ROWS>
__device__ __forceinline__ void wl_dot(const float *rows, int ldt, const WlWord &p, int sub, int rc, int nrows, float (&acc)[ROWS]) {
#pragma unroll
    for (int r = 0; r < ROWS; ++r) acc[r] = 0.0f;
    // the word's whole share of the weight row is requested before any of it is used (k <= 256: at
    // most 8 x 16 B per lane): one memory round trip per word instead of one per 32 k-values
    f32x4 bv[8];
#pragma unroll
    for (int c8 = 0; c8 < 8; ++c8) {
        const int kc = sub + 8 * c8;
        bv[c8] = (kc < p.K4 && kc < 64) ? p.brow[kc] : f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int c8 = 0; c8 < 8; ++c8) {
        const int kc = sub + 8 * c8;
        if (kc >= p.K4 || kc >= 64) continue;
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            if (rc + r < nrows) {
                const float *tv = rows + (size_t)r * ldt + p.toff + kc * 4;
                acc[r] = fmaf(bv[c8][0], tv[0], acc[r]);
                acc[r] = fmaf(bv[c8][1], tv[1], acc[r]);
                acc[r] = fmaf(bv[c8][2], tv[2], acc[r]);
                acc[r] = fmaf(bv[c8][3], tv[3], acc[r]);
            }
        }
    }
    for (int kc = sub + 64; kc < p.K4; kc += 8) {            // k > 256 (untied models): the tail
        const f32x4 bw = p.brow[kc];
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            if (rc + r < nrows) {
                const float *tv = rows + (size_t)r * ldt + p.toff + kc * 4;
                acc[r] = fmaf(bw[0], tv[0], acc[r]);
                acc[r] = fmaf(bw[1], tv[1], acc[r]);
                acc[r] = fmaf(bw[2], tv[2], acc[r]);
                acc[r] = fmaf(bw[3], tv[3], acc[r]);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < ROWS; ++r) acc[r] = wl_sum8(acc[r]);
}
