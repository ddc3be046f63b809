// jlm_ngram_edge.hip -- a back-off word n-gram model mixed into the decode's frame loop (include/jlm_hip.h jlm_ngram_cell_patch;
// DESIGN.md section 24): p = (1 - lam) p_lm + lam p_ng per hypothesis, as a rewrite of the edge-logit buffer the next beam step reads.
// Unlike the continuous cache (csrc/jlm_cache_edge.hip) the term does not depend on the hidden state but on the hypothesis's last two
// words, found through jlm_beam_state.bp / .word, and it is a look-up in a hash table resident in HBM.
//
// ngram_cell_patch_kernel -- one workgroup of 256 threads per sentence.  Wave 0 folds the cell's normaliser slices into lse with the
// beam step's own fold (csrc/jlm_beam_fold.h) while the threads of waves 1, 2, 3, 0 read a slot's history each: bp and word of its row
// in one trip, bp and word of its parent in a second (a root row: root_hist instead), then the first slots of its two context weights
// bow(u v) and bow(v) together, key and value in the same trip -- a look-up that hits its home slot is one round trip.  u, v and the
// weights stay in LDS.  Then the cell's word list 256 positions at a time: thread p looks the unigram of its position up once (LDS),
// and the (position, slot) pairs are dealt over the threads with the slot fastest, so that a wave writes consecutive edge logits:
// per pair the first slots of the trigram and of the bigram are requested together, the walk down adds the slot's weights, and the
// edge logit is rewritten in f64.  One writer per address, no atomics but the flag word's.  Every probe loop is bounded by the
// launch argument max_probe and every slot index is masked into the table, whatever the table holds.
#include <math.h>
#include "jlm_common.h"
#include "jlm_beam_fold.h"

namespace {

constexpr int NG_THREADS = 256;
constexpr unsigned long long NG_GOLDEN = 0x9E3779B97F4A7C15ull;
constexpr int NG_MAX_ID = (1 << 21) - 2;

struct NgramPatchArgs {
    const unsigned long long *keys;
    const float2 *vals;
    const int *g0, *cnt, *sent_len, *bp, *word, *root_hist, *wl, *wl_off, *wl_idx, *wl_out, *live_base;
    const double *score;
    const float *part;
    float *edge;
    double *lse;
    int *flags;
    int log2cap, max_probe, order, frame, beam, ld_part, n_parts, wl_base;
    double log1m, log_rho;             // log(1 - lambda), log(lambda / (1 - lambda))
};

__device__ __forceinline__ bool ng_id_ok(int w) { return w >= 0 && w <= NG_MAX_ID; }

// the key of (u, v, w), the predicted word lowest; an absent position (< 0) is 0
__device__ __forceinline__ unsigned long long ng_key(int u, int v, int w) {
    return (unsigned long long)(w + 1) | ((unsigned long long)(v + 1) << 21) | ((unsigned long long)(u + 1) << 42);
}

struct NgProbe {
    unsigned long long key, k0;        // the key looked for and what its home slot holds
    float2 v0;
    unsigned slot;
};

// the first trip of a look-up: key and value of the home slot, requested together
__device__ __forceinline__ NgProbe ng_first(const NgramPatchArgs &a, unsigned long long key) {
    NgProbe p;
    p.key = key;
    p.slot = (unsigned)((key * NG_GOLDEN) >> (64 - a.log2cap));
    p.k0 = a.keys[p.slot];
    p.v0 = a.vals[p.slot];
    return p;
}

// ... and the rest of it: true and the entry, or false (an empty slot, or max_probe + 1 slots seen)
__device__ __forceinline__ bool ng_finish(const NgramPatchArgs &a, const NgProbe &p, float2 &out) {
    unsigned long long k = p.k0;
    float2 v = p.v0;
    unsigned slot = p.slot;
    const unsigned mask = (1u << a.log2cap) - 1u;
    for (int i = 0;; ++i) {
        if (k == p.key) { out = v; return true; }
        if (k == 0ull || i >= a.max_probe) return false;
        slot = (slot + 1u) & mask;
        k = a.keys[slot];
        v = a.vals[slot];
    }
}

__global__ void __launch_bounds__(NG_THREADS) ngram_cell_patch_kernel(const NgramPatchArgs a) {
    extern __shared__ __attribute__((aligned(16))) double ng_lds[];   // [beam] L | int [beam] u, v | float [beam] bow(u v), bow(v) | per-position
    const int j = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (a.frame >= a.sent_len[j]) return;                          // (block-uniform, as every return below)
    const int kcnt = min(a.cnt[j], a.beam);
    if (kcnt <= 0) return;
    double *sh_L = ng_lds;
    int *sh_u = reinterpret_cast<int *>(sh_L + a.beam);
    int *sh_v = sh_u + a.beam;
    float *sh_b2 = reinterpret_cast<float *>(sh_v + a.beam);
    float *sh_b1 = sh_b2 + a.beam;
    float *sh_uni = sh_b1 + a.beam;                                // [NG_THREADS]: lp of the position's unigram, 1 for "absent"
    int *sh_w = reinterpret_cast<int *>(sh_uni + NG_THREADS);      // [NG_THREADS]: the position's word
    int *sh_out = sh_w + NG_THREADS;                               // [NG_THREADS]: ... and lattice node

    // ---- the cell's log-normalisers: the beam step's fused fold, by wave 0 (the next beam step reads lse: it runs unfused)
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
        for (int k = tid; k < kcnt; k += NG_THREADS) sh_L[k] = 0.0;
    }

    // ---- per slot: the last two words of its history and the two context weights
    const int g_first = a.g0[j], r_u = a.root_hist[2 * j], r_v = a.root_hist[2 * j + 1];
    for (int k = (tid + NG_THREADS - 64) & (NG_THREADS - 1); k < kcnt; k += NG_THREADS) {      // (slot 0 on wave 1: beside the fold)
        const int g = g_first + k;
        const int b = a.bp[g], w0 = a.word[g];                     // (one trip)
        const bool finite = a.score ? isfinite(a.score[g]) : true;
        int u, v;
        if (b < 0) {                                               // a root row consumes the context's last word, not st.word
            u = r_u;
            v = r_v;
        } else {
            const int bb = a.bp[b], wb = a.word[b];                // (a second)
            v = w0;
            u = bb < 0 ? r_v : wb;
        }
        if (a.order < 3 || !ng_id_ok(u) || !ng_id_ok(v)) u = -1;
        if (a.order < 2 || !ng_id_ok(v)) v = -1;
        float b2 = 0.0f, b1 = 0.0f;
        if (v >= 0) {
            const NgProbe p1 = ng_first(a, ng_key(-1, -1, v));
            float2 e;
            if (u >= 0) {
                const NgProbe p2 = ng_first(a, ng_key(-1, u, v));  // (both home slots in one trip)
                if (ng_finish(a, p2, e)) b2 = e.y;
            }
            if (ng_finish(a, p1, e)) b1 = e.y;
        }
        if (!finite || !isfinite(b2) || !isfinite(b1)) {           // the slot keeps its edge logits
            v = -2;
            if (a.flags) atomicOr(a.flags, 8);
        }
        sh_u[k] = u;
        sh_v[k] = v;
        sh_b2[k] = b2;
        sh_b1[k] = b1;
    }

    const int l = a.wl_base + a.wl_idx[j];                         // the cell's list, as jlm_edge_logits finds it
    const int off0 = a.wl_off[l], J = a.wl_off[l + 1] - off0;
    for (int p0 = 0; p0 < J; p0 += NG_THREADS) {
        const int n_pos = min(NG_THREADS, J - p0);
        __syncthreads();                                           // L and the slots' words are written; the last chunk's pairs are done
        if (tid < n_pos) {
            const int w = a.wl[off0 + p0 + tid];
            float lp = 1.0f;
            if (ng_id_ok(w)) {
                float2 e;
                if (ng_finish(a, ng_first(a, ng_key(-1, -1, w)), e)) lp = e.x;
            }
            sh_uni[tid] = lp;
            sh_w[tid] = w;
            sh_out[tid] = a.wl_out[off0 + p0 + tid];
        }
        __syncthreads();
        for (int t = tid; t < n_pos * kcnt; t += NG_THREADS) {
            const int pos = t / kcnt, k = t - pos * kcnt;
            const int v = sh_v[k];
            if (v == -2) continue;
            const int u = sh_u[k], w = sh_w[pos];
            float *e_out = a.edge + (size_t)sh_out[pos] * a.beam + k;
            const double y = (double)*e_out;
            const bool w_ok = ng_id_ok(w);
            double q = 0.0;
            bool found = false;
            if (w_ok && v >= 0) {
                const NgProbe p2 = ng_first(a, ng_key(-1, v, w));
                float2 e;
                if (u >= 0) {
                    const NgProbe p3 = ng_first(a, ng_key(u, v, w));   // (trigram and bigram home slots in one trip)
                    if (ng_finish(a, p3, e)) {
                        q = (double)e.x;
                        found = true;
                    } else {
                        q = (double)sh_b2[k];
                    }
                }
                if (!found) {
                    if (ng_finish(a, p2, e)) {
                        q += (double)e.x;
                        found = true;
                    } else {
                        q += (double)sh_b1[k];
                    }
                }
            }
            if (!found) {
                const float lp1 = sh_uni[pos];
                if (lp1 <= 0.0f) {
                    q += (double)lp1;
                    found = true;
                }
            }
            const double L = sh_L[k];
            const double r = found ? L + a.log1m + jlm_logaddexp(y - L, a.log_rho + q) : y + a.log1m;
            *e_out = (float)r;
        }
    }
}

}  // namespace

// the refusals of jlm_ngram_cell_patch on their own (jlm_decode_frames asks before its first launch): -1, or 0
int jlm_ngram_cell_patch_refuse(const void *keys, const float *vals, int log2cap, int max_probe, int order, float lam, const int *g0,
                                const int *cnt, const int *sent_len, int frame, int n_sent, int beam, const int *bp, const int *word,
                                const double *score, const int *root_hist, const int *wl, const int *wl_off, const int *wl_idx, int wl_base,
                                const int *wl_out, const float *edge, const float *part, int ld_part, int n_parts, const int *live_base,
                                const double *lse, const int *flags) {
    if (order < 1 || order > 3 || log2cap < 6 || log2cap > 31) return -1;
    if (max_probe < 0 || (long long)max_probe >= (1ll << log2cap)) return -1;
    if (!(lam > 0.0f && lam < 1.0f)) return -1;
    if (n_sent < 0 || frame < 0 || beam < 1 || beam > JLM_MAX_BEAM) return -1;
    if (part && (!live_base || !lse || n_parts < 1 || ld_part < 1)) return -1;
    if (!keys || !vals || (((uintptr_t)keys | (uintptr_t)vals) & 7) != 0) return -1;
    if (n_sent == 0) return 0;
    if (!g0 || !cnt || !sent_len || !bp || !word || !root_hist || !wl || !wl_off || !wl_idx || wl_base < 0 || !wl_out || !edge) return -1;
    if ((((uintptr_t)g0 | (uintptr_t)cnt | (uintptr_t)sent_len | (uintptr_t)bp | (uintptr_t)word | (uintptr_t)root_hist | (uintptr_t)wl |
          (uintptr_t)wl_off | (uintptr_t)wl_idx | (uintptr_t)wl_out | (uintptr_t)edge | (uintptr_t)live_base | (uintptr_t)flags) & 3) != 0)
        return -1;
    if ((((uintptr_t)part | (uintptr_t)lse | (uintptr_t)score) & 7) != 0) return -1;
    return 0;
}

extern "C" int jlm_ngram_cell_patch(const void *keys, const float *vals, int log2cap, int max_probe, int order, float lam, const int *g0,
                                    const int *cnt, const int *sent_len, int frame, int n_sent, int beam, const int *bp, const int *word,
                                    const double *score, const int *root_hist, const int *wl, const int *wl_off, const int *wl_idx,
                                    int wl_base, const int *wl_out, float *edge, const float *part, int ld_part, int n_parts,
                                    const int *live_base, double *lse, int *flags, void *stream) {
    if (int rc = jlm_ngram_cell_patch_refuse(keys, vals, log2cap, max_probe, order, lam, g0, cnt, sent_len, frame, n_sent, beam, bp, word,
                                             score, root_hist, wl, wl_off, wl_idx, wl_base, wl_out, edge, part, ld_part, n_parts,
                                             live_base, lse, flags))
        return rc;
    if (n_sent == 0) return 0;
    NgramPatchArgs a;
    a.keys = (const unsigned long long *)keys; a.vals = (const float2 *)vals; a.g0 = g0; a.cnt = cnt; a.sent_len = sent_len; a.bp = bp;
    a.word = word; a.root_hist = root_hist; a.wl = wl; a.wl_off = wl_off; a.wl_idx = wl_idx; a.wl_out = wl_out; a.live_base = live_base;
    a.score = score; a.part = part; a.edge = edge; a.lse = lse; a.flags = flags; a.log2cap = log2cap; a.max_probe = max_probe;
    a.order = order; a.frame = frame; a.beam = beam; a.ld_part = ld_part; a.n_parts = n_parts; a.wl_base = wl_base;
    a.log1m = log1p(-(double)lam);
    a.log_rho = log((double)lam) - log1p(-(double)lam);
    const size_t lds = (size_t)beam * (8 + 4 * 4) + (size_t)NG_THREADS * 12;      // 27 KB at most (beam 1 024)
    ngram_cell_patch_kernel<<<dim3(n_sent), dim3(NG_THREADS), lds, (hipStream_t)stream>>>(a);
    return (int)hipGetLastError();
}
