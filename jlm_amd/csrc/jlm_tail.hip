// Prediction of an unfinished last word behind a static decode (Decoder.decode_predict): one launch per batch,
// one workgroup per sentence, behind jlm_decode_frames on the batch's stream.
//
// The decode leaves, for every frame s < sentence length, the surviving hypotheses' T rows, scores and log-normalisers in the plan's
// pools.  A *span* (frame, lo, hi) names the words ids[lo .. hi) -- a contiguous piece of the vocabulary sorted by (reading, id):
// the words whose reading properly extends the input's tail from `frame` on.  A candidate is (span, word, slot < cnt(frame)); its
// score is score[g] + lse[g] - logit(row g, word) in f64 (self-normalised models: score[g] - logit), and the n_out best by
// (score, candidate index) are written with their parents' back-traces.  Candidate index = position in (span, word, slot) order.
//
// Logits: wl_lookup and wl_dot of csrc/jlm_wordlist_dot.h, the functions wordlist_kernel (csrc/jlm_beam.hip) calls, then + b2[w] -- so a
// candidate's logit is bit-equal to what jlm_edge_logits gives for that (row, word).  The rows of a span's frame are staged TP_ROWS at
// a time, as there.
//
// Selection: candidates are appended to an LDS buffer as they are formed (every position has one writer: no atomics); whenever `chunk`
// of them are waiting they are selected together with the n_out winners carried so far, and the winners are carried on -- LDS is
// n_out + chunk + one word block of candidates whatever the candidate count.  The order is the lexicographic (score, candidate index)
// minimum throughout and a candidate index is unique, so the result depends neither on `chunk` nor on the order of formation.
// A NaN score never compares below anything: it never ranks.
#include "jlm_common.h"
#include "jlm_wave.h"
#include "jlm_wordlist_dot.h"

#define TP_THREADS 256
#define TP_ROWS 16                                 // hypothesis rows per pass (WL_ROWS of wordlist_kernel)
#define TP_BLOCK (TP_THREADS / 8 * TP_ROWS)        // candidates one word block (32 words x TP_ROWS rows) can add
#define TP_MAX_OUT 64
#define TP_DEFAULT_CHUNK 4096
#define TP_NONE 0x7fffffff

struct TailArgs {
    SegTable segs;
    const float *b2, *T;
    int ldt, n_sent, beam, n_frames;
    const double *score, *lse;
    const int *cnt, *bp, *node;
    int mode;
    const int *ids;
    int n_ids;
    const int *sp_off, *sp_frame, *sp_lo, *sp_hi;
    int n_out, chunk;
    double *out_score;
    int *out_row, *out_word, *out_nodes, *out_len;
    int stride;
};

// a span the kernel serves: its frame inside the plan, its words inside ids[], not empty
__device__ __forceinline__ bool tp_span_ok(const TailArgs &a, int f, int lo, int hi) {
    return f >= 0 && f < a.n_frames && lo >= 0 && lo < hi && hi <= a.n_ids;
}

// The n_out best of key[0 .. n) / cix[0 .. n) by (key, candidate index) -> key / cix [0 .. n_out), best first; the rest of the region is
// dead afterwards.  Thread t owns entries t, t + 256, ...: it carries the minimum of its own entries in registers, a round is a
// workgroup-wide arg-min over those 256 pairs (DPP inside a wave, the four waves through LDS, one barrier: the scratch alternates), after
// which only the winner's owner strikes its entry and rescans.  Every thread of the workgroup calls this with the same arguments.
__device__ void tp_select(double *key, int *cix, int n, int n_out, double *win_v, int *win_c, double *red_v, int *red_c) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const double INF = __longlong_as_double(0x7ff0000000000000LL);
    double bv = INF;
    int bc = TP_NONE, bp = -1;
    for (int i = tid; i < n; i += TP_THREADS) {
        const double v = key[i];
        const int c = cix[i];
        if (v < bv || (v == bv && c < bc)) { bv = v; bc = c; bp = i; }
    }
    for (int r = 0; r < n_out; ++r) {
        double v = bv;
        int c = bc;
        wave_argmin(v, c);
        const int o = (r & 1) * (TP_THREADS / 64);
        if (lane == 0) { red_v[o + wave] = v; red_c[o + wave] = c; }
        __syncthreads();
        v = red_v[o];
        c = red_c[o];
#pragma unroll
        for (int w2 = 1; w2 < TP_THREADS / 64; ++w2) {
            const double v2 = red_v[o + w2];
            const int c2 = red_c[o + w2];
            if (v2 < v || (v2 == v && c2 < c)) { v = v2; c = c2; }
        }
        if (tid == 0) { win_v[r] = v; win_c[r] = c; }
        if (c != TP_NONE && c == bc) {                 // a candidate index is unique: this thread owns the winner
            key[bp] = INF;
            cix[bp] = TP_NONE;
            bv = INF; bc = TP_NONE; bp = -1;
            for (int i = tid; i < n; i += TP_THREADS) {
                const double v2 = key[i];
                const int c2 = cix[i];
                if (v2 < bv || (v2 == bv && c2 < bc)) { bv = v2; bc = c2; bp = i; }
            }
        }
    }
    __syncthreads();                                   // every owner's last strike, the winners
    if (tid < n_out) { key[tid] = win_v[tid]; cix[tid] = win_c[tid]; }
    __syncthreads();
}

__global__ __launch_bounds__(TP_THREADS) void tail_predict_kernel(TailArgs a) {
    // rows [TP_ROWS x ldt] f32 (16-byte pieces; 64 ldt bytes) | 8-byte arrays: key [cap], rowsc [TP_ROWS], win_v [64], red_v [8] |
    // 4-byte arrays: cix [cap], win_c [64], red_c [8]
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int s = blockIdx.x, tid = threadIdx.x;
    const int B = a.n_sent, beam = a.beam, rmax = B * beam, ldt = a.ldt;
    const int n_out = a.n_out, chunk = a.chunk, cap = n_out + chunk + TP_BLOCK;
    const double INF = __longlong_as_double(0x7ff0000000000000LL);
    double *key = reinterpret_cast<double *>(sm + (size_t)TP_ROWS * ldt);
    double *rowsc = key + cap;
    double *win_v = rowsc + TP_ROWS;
    double *red_v = win_v + TP_MAX_OUT;
    int *cix = reinterpret_cast<int *>(red_v + 2 * (TP_THREADS / 64));
    int *win_c = cix + cap;
    int *red_c = win_c + TP_MAX_OUT;
    const int sub = tid & 7, slot = tid >> 3;
    if (tid < n_out) { key[tid] = INF; cix[tid] = TP_NONE; }      // the winners carried so far: none
    int fill = n_out;                                              // entries of key / cix in use (the same in every thread)
    int cbase = 0;                                                 // candidate index of the span's first candidate
    const int sp0 = a.sp_off[s], sp1 = a.sp_off[s + 1];
    for (int sp = sp0; sp < sp1; ++sp) {
        const int f = a.sp_frame[sp], lo = a.sp_lo[sp], hi = a.sp_hi[sp];
        if (!tp_span_ok(a, f, lo, hi)) continue;
        const int nrows = min(a.cnt[f * B + s], beam);
        if (nrows <= 0) continue;
        const int nw = hi - lo;
        const int gbase = f * rmax + s * beam;
        for (int rc = 0; rc < nrows; rc += TP_ROWS) {
            const int nr = min(TP_ROWS, nrows - rc);
            {   // stage this pass's rows T[gbase + rc .. + nr) and their score + lse (behind every reader of the pass before)
                __syncthreads();
                const f32x4 *src = reinterpret_cast<const f32x4 *>(a.T + (size_t)(gbase + rc) * ldt);
                f32x4 *dst = reinterpret_cast<f32x4 *>(sm);
                for (int i = tid; i < nr * (ldt / 4); i += TP_THREADS) dst[i] = src[i];
                if (tid < nr) {
                    const int g = gbase + rc + tid;
                    rowsc[tid] = a.mode == 1 ? a.score[g] : a.score[g] + a.lse[g];
                }
                __syncthreads();
            }
            for (int wb = 0; wb < nw; wb += TP_THREADS / 8) {
                const int wi = wb + slot;
                const bool valid = wi < nw;
                const int w = valid ? a.ids[lo + wi] : -1;
                float acc[TP_ROWS];
                wl_dot<TP_ROWS>(sm, ldt, wl_lookup(a.segs, w, valid), sub, 0, nr, acc);
                // the block's candidates: words wb .. wb + nwb, rows rc .. rc + nr, word-major behind what is waiting
                const int nwb = min(TP_THREADS / 8, nw - wb);
                if (valid && sub == 0) {
                    const float bw = a.b2[w];
                    const int p0 = fill + slot * nr, c0 = cbase + wi * nrows + rc;
#pragma unroll
                    for (int r = 0; r < TP_ROWS; ++r) {
                        if (r < nr) {
                            const float y = acc[r] + bw;
                            key[p0 + r] = rowsc[r] - (double)y;
                            cix[p0 + r] = c0 + r;
                        }
                    }
                }
                fill += nwb * nr;
                while (fill - n_out >= chunk) {                    // `chunk` candidates are waiting: select them with the winners so far
                    __syncthreads();
                    tp_select(key, cix, n_out + chunk, n_out, win_v, win_c, red_v, red_c);
                    // what was formed behind the chunk (less than one word block) moves up behind the winners
                    const int left = fill - (n_out + chunk);
                    double mv[TP_BLOCK / TP_THREADS];
                    int mc[TP_BLOCK / TP_THREADS];
#pragma unroll
                    for (int j = 0; j < TP_BLOCK / TP_THREADS; ++j) {
                        const int i = tid + j * TP_THREADS;
                        if (i < left) { mv[j] = key[n_out + chunk + i]; mc[j] = cix[n_out + chunk + i]; }
                    }
                    __syncthreads();
#pragma unroll
                    for (int j = 0; j < TP_BLOCK / TP_THREADS; ++j) {
                        const int i = tid + j * TP_THREADS;
                        if (i < left) { key[n_out + i] = mv[j]; cix[n_out + i] = mc[j]; }
                    }
                    fill = n_out + left;
                }
            }
        }
        cbase += nw * nrows;
    }
    __syncthreads();
    if (fill > n_out) tp_select(key, cix, fill, n_out, win_v, win_c, red_v, red_c);
    // ---- rank r's candidate: its span, word and slot from the candidate index; the parent's trace as jlm_backtrace writes it
    if (tid < n_out) {
        const size_t o = (size_t)s * n_out + tid;
        const int c = cix[tid];
        int g = -1, word = -1;
        if (c != TP_NONE) {
            int base = 0;
            for (int sp = sp0; sp < sp1; ++sp) {
                const int f = a.sp_frame[sp], lo = a.sp_lo[sp], hi = a.sp_hi[sp];
                if (!tp_span_ok(a, f, lo, hi)) continue;
                const int nrows = min(a.cnt[f * B + s], beam);
                if (nrows <= 0) continue;
                const int n = (hi - lo) * nrows;
                if (c < base + n) {
                    const int rem = c - base;
                    word = a.ids[lo + rem / nrows];
                    g = f * rmax + s * beam + rem % nrows;
                    break;
                }
                base += n;
            }
        }
        a.out_score[o] = g >= 0 ? key[tid] : INF;
        a.out_row[o] = g;
        a.out_word[o] = word;
        int d = 0;
        while (g >= 0 && d < a.stride) {
            a.out_nodes[o * a.stride + d] = a.node[g];
            ++d;
            g = a.bp[g];
        }
        a.out_len[o] = d;
    }
}

static size_t tail_lds_bytes(int ldt, int n_out, int chunk) {
    const size_t cap = (size_t)n_out + chunk + TP_BLOCK;
    return (size_t)TP_ROWS * ldt * sizeof(float) + (cap + TP_ROWS + TP_MAX_OUT + 2 * (TP_THREADS / 64)) * sizeof(double) +
           (cap + TP_MAX_OUT + 2 * (TP_THREADS / 64)) * sizeof(int);
}

extern "C" int jlm_tail_predict(const jlm_segment *segs_host, int n_segs, const float *b2, const float *T, int ldt, int n_sent, int beam,
                                int n_frames, const double *score, const double *lse, const int *cnt, const int *bp, const int *node,
                                int mode, const int *ids, int n_ids, const int *sp_off, const int *sp_frame, const int *sp_lo,
                                const int *sp_hi, int n_out, int chunk, double *out_score, int *out_row, int *out_word, int *out_nodes,
                                int *out_len, int stride, void *stream) {
    TailArgs a;
    if (n_segs < 1 || n_segs > JLM_MAX_SEGMENTS || !segs_host) return -1;
    a.segs.n = n_segs;
    for (int i = 0; i < n_segs; ++i) {
        a.segs.s[i] = segs_host[i];
        if (a.segs.s[i].k % 4 || a.segs.s[i].ldb % 4 || a.segs.s[i].t_off % 4 || !a.segs.s[i].B) return -1;
    }
    if (n_out < 1 || n_out > TP_MAX_OUT || beam < 1 || beam > JLM_MAX_BEAM || ldt < 4 || ldt % 4 || n_frames < 1 || stride < 1 ||
        mode < 0 || mode > 1 || chunk < 0 || n_ids < 0)
        return -1;
    if (!b2 || !T || !score || (mode == 0 && !lse) || !cnt || !bp || !node || !ids || !sp_off || !sp_frame || !sp_lo || !sp_hi ||
        !out_score || !out_row || !out_word || !out_nodes || !out_len)
        return -1;
    if (n_sent <= 0) return 0;
    if (chunk == 0) chunk = TP_DEFAULT_CHUNK;
    const size_t lds = tail_lds_bytes(ldt, n_out, chunk);
    if (lds > 160 * 1024) return -1;
    a.b2 = b2; a.T = T; a.ldt = ldt; a.n_sent = n_sent; a.beam = beam; a.n_frames = n_frames;
    a.score = score; a.lse = lse; a.cnt = cnt; a.bp = bp; a.node = node; a.mode = mode;
    a.ids = ids; a.n_ids = n_ids; a.sp_off = sp_off; a.sp_frame = sp_frame; a.sp_lo = sp_lo; a.sp_hi = sp_hi;
    a.n_out = n_out; a.chunk = chunk;
    a.out_score = out_score; a.out_row = out_row; a.out_word = out_word; a.out_nodes = out_nodes; a.out_len = out_len; a.stride = stride;
    static JlmLdsGrant grant;
    if (int rc = jlm_grant_lds(grant, reinterpret_cast<const void *>(tail_predict_kernel), (int)lds)) return rc;
    hipLaunchKernelGGL(tail_predict_kernel, dim3(n_sent), dim3(TP_THREADS), lds, (hipStream_t)stream, a);
    JLM_LAUNCH_CHECK();
    return 0;
}
