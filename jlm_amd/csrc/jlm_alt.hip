// Per-segment candidate lists behind a static decode (Decoder.decode_candidates): the head launch, one workgroup
// per sentence, once the batch's jlm_decode_frames has completed, in front of jlm_score_frames' launches over the same rows.
//
// The decode leaves every frame's surviving hypotheses in the plan's pools: state rows (h, c), projection rows T, scores and
// log-normalisers, row g = frame * rmax + s * beam + k.  Path `rank` of sentence s is the chain g_K, bp[g_K], ... down to the root g_0
// (bp = -1), walked here from the final row sent_len[s] * rmax + s * beam + rank: no pool row index comes from the host.  A row r of the
// call names (sentence, depth d = k - 1, word a): word a put into segment k of that path.  For it the kernel
//   1. forms logit(T[g_d], a) with wl_lookup and wl_dot of csrc/jlm_wordlist_dot.h, the functions wordlist_kernel (csrc/jlm_beam.hip)
//      and tail_predict_kernel (csrc/jlm_tail.hip) call, then + b2[a] -- so it is bit-equal to what jlm_edge_logits gives for that
//      (row, word);
//   2. seeds the accumulator jlm_score_frames adds the suffix terms to:  nll_seq[r] = head + (score[g_K] - score[g_{k+j}])  in f64,
//      head = score[g_d] + lse[g_d] - logit (mode 1, self-normalised: score[g_d] - logit), j = the row's suffix steps = the number of
//      steps t with n_live[t] > r;
//   3. for j >= 1 copies the state rows (h, c)[g_d] byte for byte into row r of row set 0, and writes prev0[r] = r.
// The path's T rows are staged AH_ROWS depths at a time: LDS is AH_ROWS rows of T, the path (n_frames entries) and the live counts,
// whatever the beam.  Plain vector loads and stores, one writer per address, no atomics but the flag word's OR.
#include "jlm_common.h"
#include "jlm_wordlist_dot.h"

#define AH_THREADS 256
#define AH_ROWS 16                                 // path rows staged per pass

struct AltArgs {
    SegTable segs;
    const float *b2, *T;
    int ldt, n_sent, beam, n_frames, mode, rank, rec;
    const double *score, *lse;
    const int *bp, *sent_len;
    const uint4 *src_h, *src_c;
    const int *sent_off, *sent_rows, *depth, *alt, *n_live;
    int n_rows, n_steps;
    uint4 *dst_h, *dst_c;
    int *prev0;
    double *nll_seq;
    int *flags;
};

__global__ __launch_bounds__(AH_THREADS) void alt_head_kernel(AltArgs a) {
    // rows [AH_ROWS x ldt] f32 | 8-byte arrays: psc [n_frames], base [AH_ROWS] | 4-byte arrays: pg [n_frames], live [n_steps], meta [2]
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int s = blockIdx.x, tid = threadIdx.x;
    const int beam = a.beam, rmax = a.n_sent * beam, ldt = a.ldt, P = a.n_frames, S = a.n_steps;
    const long long G = (long long)P * rmax;
    const double INF = __longlong_as_double(0x7ff0000000000000LL);
    double *psc = reinterpret_cast<double *>(sm + (size_t)AH_ROWS * ldt);      // (psc and pg move up to the path's first entry below)
    double *base = psc + P;
    int *pg = reinterpret_cast<int *>(base + AH_ROWS);
    int *live = pg + P;
    int *meta = live + S;
    const int sub = tid & 7, slot = tid >> 3;
    const int i0 = a.sent_off[s], i1 = a.sent_off[s + 1];
    if (i0 < 0 || i1 > a.n_rows || i0 >= i1) return;              // a sentence without rows (the same in every thread)
    for (int t = tid; t < S; t += AH_THREADS) live[t] = a.n_live[t];
    if (tid == 0) {
        // the path in ONE walk from the final row down: written from the arrays' ends backwards, so that it stands root first at offset
        // P - n once its length n is known -- pg[off .. off + K], psc their scores.  K = -1: the walk left the pool
        const int L = a.sent_len[s];
        bool ok = L >= 1 && L < P;
        int n = 0;
        long long g = (long long)L * rmax + (long long)s * beam + a.rank;
        while (ok && g != -1) {
            if (g < 0 || g >= G || n >= P) { ok = false; break; }
            ++n;
            pg[P - n] = (int)g;
            psc[P - n] = a.score[g];
            g = a.bp[g];
        }
        if (n < 1) ok = false;
        meta[0] = ok ? n - 1 : -1;
        meta[1] = P - n;
    }
    __syncthreads();
    const int K = meta[0];
    pg += meta[1];
    psc += meta[1];
    if (K < 0) {
        for (int i = i0 + tid; i < i1; i += AH_THREADS) {
            const int r = a.sent_rows[i];
            if (r < 0 || r >= a.n_rows) continue;
            a.nll_seq[r] = INF;
            a.prev0[r] = -1;
        }
        if (tid == 0 && a.flags) atomicOr(a.flags, 4);
        return;
    }
    for (int d0 = 0; d0 == 0 || d0 < K; d0 += AH_ROWS) {
        const int nr = max(0, min(AH_ROWS, K - d0));
        {   // stage this pass's rows T[pg[d0 .. d0 + nr)] and their score + lse (behind every reader of the pass before)
            __syncthreads();
            const int q = ldt / 4;
            f32x4 *dst = reinterpret_cast<f32x4 *>(sm);
            for (int i = tid; i < nr * q; i += AH_THREADS) {
                const int row = i / q;
                dst[i] = reinterpret_cast<const f32x4 *>(a.T + (size_t)pg[d0 + row] * ldt)[i - row * q];
            }
            if (tid < nr) {
                const int g = pg[d0 + tid];
                double b = psc[d0 + tid];
                if (a.mode != 1) {
                    const double l = a.lse[g];
                    if (!(fabs(l) < 1.0e300) && a.flags) atomicOr(a.flags, 1);
                    b += l;
                }
                base[tid] = b;
            }
            __syncthreads();
        }
        for (int ib = i0; ib < i1; ib += AH_THREADS / 8) {
            const int i = ib + slot;
            int r = i < i1 ? a.sent_rows[i] : -1;
            if (r >= a.n_rows) r = -1;
            const int d = r >= 0 ? a.depth[r] : -1;
            int j = 0;                                             // #{t : live[t] > r}: live[] does not increase
            for (int hi = r >= 0 ? S : 0; j < hi;) {
                const int mid = (j + hi) >> 1;
                if (live[mid] > r) j = mid + 1; else hi = mid;
            }
            const bool broken = r >= 0 && (d < 0 || d >= K || d + 1 + j > K);       // fewer segments than the row's depth
            const bool valid = r >= 0 && !broken && d >= d0 && d < d0 + nr;
            const int w = valid ? a.alt[r] : -1;
            const WlWord p = wl_lookup(a.segs, w, valid);
            const bool found = p.brow != nullptr;
            float acc[1];
            wl_dot<1>(sm + (size_t)(valid ? d - d0 : 0) * ldt, ldt, p, sub, 0, 1, acc);
            if (broken && d0 == 0 && sub == 0) {
                a.nll_seq[r] = INF;
                a.prev0[r] = -1;
                if (a.flags) atomicOr(a.flags, 4);
            }
            if (!valid) continue;
            if (sub == 0) {
                if (found) {
                    const float y = acc[0] + a.b2[w];
                    const double head = base[d - d0] - (double)y;
                    a.nll_seq[r] = head + (psc[K] - psc[d + 1 + j]);
                } else {                                           // a word in no segment: NaN, nothing of B or b2 is read
                    a.nll_seq[r] = __longlong_as_double(0x7ff8000000000000LL);
                    if (a.flags) atomicOr(a.flags, 2);
                }
                a.prev0[r] = r;
            }
            if (j >= 1) {
                const size_t from = (size_t)pg[d] * a.rec, to = (size_t)r * a.rec;
                for (int c = sub; c < a.rec; c += 8) {
                    a.dst_h[to + c] = a.src_h[from + c];
                    a.dst_c[to + c] = a.src_c[from + c];
                }
            }
        }
    }
}

static size_t alt_lds_bytes(int ldt, int n_frames, int n_steps) {
    return (size_t)AH_ROWS * ldt * sizeof(float) + ((size_t)n_frames + AH_ROWS) * sizeof(double) +
           ((size_t)n_frames + n_steps + 2) * sizeof(int);
}

extern "C" int jlm_alt_head_refuse(const jlm_segment *segs_host, int n_segs, const float *b2, int ldt, int H, int mode,
                                   const jlm_alt_plan *a, const jlm_score_plan *p) {
    if (!a || !p || !segs_host || n_segs < 1 || n_segs > JLM_MAX_SEGMENTS) return -1;
    for (int i = 0; i < n_segs; ++i)
        if (segs_host[i].k % 4 || segs_host[i].ldb % 4 || segs_host[i].t_off % 4 || !segs_host[i].B || ((uintptr_t)segs_host[i].B & 15))
            return -1;
    if (a->beam < 1 || a->beam > JLM_MAX_BEAM || ldt < 4 || ldt % 4 || H < 4 || H % 4 || a->n_frames < 1 || mode < 0 || mode > 1 ||
        a->rank < 0 || a->rank >= a->beam || a->n_sent < 0 || p->n_rows < 0 || p->n_steps < 0)
        return -1;
    if (a->n_sent == 0 || p->n_rows == 0) return 0;
    if ((long long)a->n_frames * a->n_sent * a->beam >= 0x7fffffffll) return -1;
    if (!b2 || !a->T || !a->h || !a->c || !a->score || (mode == 0 && !a->lse) || !a->bp || !a->sent_len || !a->sent_off || !a->sent_rows ||
        !a->depth || !a->alt || !a->prev0 || a->prev0 != p->prev0 || !p->h[0] || !p->c[0] || !p->nll_seq || (p->n_steps > 0 && !p->n_live))
        return -1;
    if ((((uintptr_t)a->T | (uintptr_t)a->h | (uintptr_t)a->c | (uintptr_t)p->h[0] | (uintptr_t)p->c[0]) & 15) != 0) return -1;
    if ((((uintptr_t)a->score | (uintptr_t)a->lse | (uintptr_t)p->nll_seq) & 7) != 0) return -1;
    if ((((uintptr_t)b2 | (uintptr_t)a->bp | (uintptr_t)a->sent_len | (uintptr_t)a->sent_off | (uintptr_t)a->sent_rows | (uintptr_t)a->depth |
          (uintptr_t)a->alt | (uintptr_t)a->prev0 | (uintptr_t)p->n_live | (uintptr_t)p->flags) & 3) != 0)
        return -1;
    if (alt_lds_bytes(ldt, a->n_frames, p->n_steps) > 160 * 1024) return -1;
    return 0;
}

extern "C" int jlm_alt_head(const jlm_segment *segs_host, int n_segs, const float *b2, int ldt, int H, int mode, const jlm_alt_plan *ap,
                            const jlm_score_plan *p, void *stream) {
    if (int rc = jlm_alt_head_refuse(segs_host, n_segs, b2, ldt, H, mode, ap, p)) return rc;
    if (ap->n_sent == 0 || p->n_rows == 0) return 0;
    AltArgs a;
    a.segs.n = n_segs;
    for (int i = 0; i < n_segs; ++i) a.segs.s[i] = segs_host[i];
    a.b2 = b2; a.T = ap->T; a.ldt = ldt; a.n_sent = ap->n_sent; a.beam = ap->beam; a.n_frames = ap->n_frames; a.mode = mode;
    a.rank = ap->rank; a.rec = H / 4;
    a.score = ap->score; a.lse = ap->lse; a.bp = ap->bp; a.sent_len = ap->sent_len;
    a.src_h = (const uint4 *)ap->h; a.src_c = (const uint4 *)ap->c;
    a.sent_off = ap->sent_off; a.sent_rows = ap->sent_rows; a.depth = ap->depth; a.alt = ap->alt; a.n_live = p->n_live;
    a.n_rows = p->n_rows; a.n_steps = p->n_steps;
    a.dst_h = (uint4 *)p->h[0]; a.dst_c = (uint4 *)p->c[0]; a.prev0 = ap->prev0; a.nll_seq = p->nll_seq; a.flags = p->flags;
    const size_t lds = alt_lds_bytes(ldt, ap->n_frames, p->n_steps);
    static JlmLdsGrant grant;
    if (int rc = jlm_grant_lds(grant, reinterpret_cast<const void *>(alt_head_kernel), (int)lds)) return rc;
    hipLaunchKernelGGL(alt_head_kernel, dim3(ap->n_sent), dim3(AH_THREADS), lds, (hipStream_t)stream, a);
    JLM_LAUNCH_CHECK();
    return 0;
}
