// The fold of the vocabulary kernel's (max, sum exp) slices into a cell's log-normalisers, shared by both beam-step kernels
// (csrc/jlm_beam.hip: the fused K6 tail) and cache_cell_patch_kernel (csrc/jlm_cache_edge.hip), which has to leave the very same bits.
#pragma once
#include "jlm_common.h"

// The fused fold of both beam-step kernels: the kprev rows of the previous cell sit at part[p * ld_part + base + r], p < n_parts; their
// log-normalisers go to lse_new[r] (LDS) and lse_out[r].  8 lanes per row, 16 rows per pass (two rows a lane), and the slices of a lane
// are requested BEAM_FOLD_NB per row at a time before any is used: one memory round trip per 8 * BEAM_FOLD_NB = 32 slices and 16 rows
// where a load per slice, each waited for, made ceil(n_parts / 8) round trips per 8 rows (the loads never depended on one another).
// A load past the end is clamped onto the last slice / row and its value dropped, so the batch is straight-line code.  The arithmetic
// and its order are what they were -- per lane the slices sub, sub + 8, ... ascending, then the xor tree 4, 2, 1 -- with the one
// rounding the compiler was free to choose written out: the new term's product is rounded, the running sum's is fused (what the
// per-slice loop compiled to).
#define BEAM_FOLD_NB 4
__device__ __forceinline__ void beam_fold_parts(const jlm_beam_state &st, int lane, int kprev, int base, double *lse_new,
                                                double *lse_out) {
    const float2 *part = reinterpret_cast<const float2 *>(st.lse_part);
    const int sub = lane & 7, n_parts = st.n_parts;
    for (int r0 = 0; r0 < kprev; r0 += 16) {
        int r[2];
        const float2 *row[2];
        float m[2];
        double sm[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            r[h] = r0 + 8 * h + (lane >> 3);
            row[h] = part + base + min(r[h], kprev - 1);
            m[h] = JLM_NEG_BIG;
            sm[h] = 0.0;
        }
        for (int pb = 0; pb < n_parts; pb += 8 * BEAM_FOLD_NB) {
            float2 v[2][BEAM_FOLD_NB];
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int j = 0; j < BEAM_FOLD_NB; ++j) v[h][j] = row[h][(size_t)min(pb + sub + 8 * j, n_parts - 1) * st.ld_part];
            __builtin_amdgcn_sched_barrier(0);             // every load of the batch is requested before the first is folded
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int j = 0; j < BEAM_FOLD_NB; ++j)
                    if (r[h] < kprev && pb + sub + 8 * j < n_parts) {
                        const float mm = fmaxf(m[h], v[h][j].x);
                        sm[h] = fma(sm[h], (double)expf(m[h] - mm), __dmul_rn((double)v[h][j].y, (double)expf(v[h][j].x - mm)));
                        m[h] = mm;
                    }
            // every load of the batch has been used or dropped: said out loud (vmcnt(0), the other counters open), so that the
            // compiler need not guard the next batch's registers with a wait at the loop's head -- that wait would also stand in
            // front of the FIRST batch and hold it back for whatever load the caller has in flight
            __builtin_amdgcn_s_waitcnt(0x0F70);
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (r0 + 8 * h >= kprev) break;                // (wave-uniform: the shuffles below are taken by all lanes or none)
            float mh = m[h];
            double sh = sm[h];
#pragma unroll
            for (int off = 4; off >= 1; off >>= 1) {
                const float m2 = __shfl_xor(mh, off);
                const double s2 = __shfl_xor(sh, off);
                const float mm = fmaxf(mh, m2);
                sh = fma(sh, (double)expf(mh - mm), __dmul_rn(s2, (double)expf(m2 - mm)));
                mh = mm;
            }
            if (sub == 0 && r[h] < kprev) {
                double l = (double)mh + log(sh);
                // inf / nan (jlm_beam_state.flags): the batch is flagged and the value replaced by a finite one -- a NaN key would leave
                // the selection rounds without a winner and the next LSTM step with garbage row indices
                if (!(fabs(l) < 1.0e300)) { if (st.flags) atomicOr(st.flags, 1); l = 1.0e30; }
                lse_new[r[h]] = l;
                lse_out[r[h]] = l;
            }
        }
    }
}
