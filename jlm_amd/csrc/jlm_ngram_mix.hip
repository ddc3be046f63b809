// jlm_ngram_mix.hip -- the back-off n-gram model on the ranking / prediction side (include/jlm_hip.h jlm_ngram_mix_rows; DESIGN.md
// section 26): q(. | history) over EVERY word of a row, as a patch of the row's materialised logits, so that rank_rows_kernel,
// topk_rows_kernel and topk_rows_masked_kernel run unchanged on the mixture -- what csrc/jlm_cache_mix.hip is to the continuous cache.
// The decode's kernel (csrc/jlm_ngram_edge.hip) looks single (history, word) pairs up in a hash table; over V words a row that would
// be V dependent probes, so this one walks the table the other way round: the successor lists of the row's contexts, longest first,
// over a dense unigram base.
//
// ngram_mix_rows_kernel -- one workgroup of 256 threads per live row.  Thread 0 resolves the row's contexts -- bow(v) and the bigram
// range of v in one trip, the home slot of (u, v) in the context map in the same trip, the trigram range and bow(u v) in a second --
// while the other threads clear the bitmap and all of them form L by rl_row (csrc/jlm_row_lse.h: the function topk_rows_kernel's
// log-normaliser is built from and cache_mix_rows_kernel calls too), read before any word is patched.  Then three passes, a barrier between
// them: the trigram successors (q = lp), the bigram successors no trigram covered (q = bow(u v) + lp), every remaining word with a
// unigram (q = (bow(u v) + bow(v)) + lp).  A bitmap of V bits in LDS, set by integer OR, says which words are done: the thread whose
// OR set the bit is the word's one writer, and it reads the original y[w].  No float atomics; every index read from the table is
// checked against a launch argument before use and every loop is bounded by one.
//
// ngram_hist_advance_kernel -- the histories behind a beam merge: hist_out[q] = (hist_in[prev_row[q]][1], word[q]).
#include <math.h>
#include "jlm_common.h"
#include "jlm_row_lse.h"

namespace {

constexpr int NM_THREADS = 256;
constexpr int NM_WAVES = NM_THREADS / 64;
constexpr int NM_DEPTH = 8;            // words a thread has in flight in the unigram pass
constexpr unsigned long long NM_GOLDEN = 0x9E3779B97F4A7C15ull;

static_assert(NM_WAVES == RL_WAVES, "rl_row (csrc/jlm_row_lse.h) is called by a workgroup of RL_WAVES waves");

struct NmArgs {
    float *y;
    jlm_ngram_rows t;
    const int *hist, *n_dev;
    int *flags;
    int ld_y, V, n_rows, order;
    float log_rho;                     // log(lambda / (1 - lambda))
};

// the context index of (u, v), or -1: the home slot's key and value are requested together, a probe stops on the key, on an empty
// slot, or after max_probe + 1 slots; every slot index is masked into the map
__device__ __forceinline__ int nm_context(const jlm_ngram_rows &t, int u, int v) {
    const unsigned long long *keys = (const unsigned long long *)t.ctx_keys;
    const unsigned long long key = (unsigned long long)(v + 1) | ((unsigned long long)(u + 1) << 21);
    const unsigned mask = (1u << t.log2cap) - 1u;
    unsigned slot = (unsigned)((key * NM_GOLDEN) >> (64 - t.log2cap)) & mask;
    unsigned long long k = keys[slot];
    int c = t.ctx_vals[slot];
    for (int i = 0;; ++i) {
        if (k == key) return c;
        if (k == 0ull || i >= t.max_probe) return -1;
        slot = (slot + 1u) & mask;
        k = keys[slot];
        c = t.ctx_vals[slot];
    }
}

// logaddexp(yw, t) of a logit and the n-gram term t = base + q; false: the word keeps its bits (t or yw is not a number to mix)
__device__ __forceinline__ bool nm_mix(float yw, float t, float &out) {
    if (!(t > -INFINITY && t < INFINITY && yw == yw)) return false;
    out = jlm_logaddexpf(yw, t);
    return true;
}

// word w of the row takes the n-gram term: the caller is its one writer
__device__ __forceinline__ void nm_patch(float *yrow, int w, float base, float q) {
    float out;
    if (nm_mix(yrow[w], base + q, out)) yrow[w] = out;
}

// one successor list [i0, i1) of (word, lp): every word not yet done is marked and patched with q = add + lp
__device__ __forceinline__ void nm_list(const int *__restrict__ ws, const float *__restrict__ lps, int i0, int i1, int V, unsigned *bits,
                                        float *yrow, float base, float add) {
    for (int i = i0 + (int)threadIdx.x; i < i1; i += NM_THREADS) {
        const int w = ws[i];
        const float lp = lps[i];
        if (w < 0 || w >= V) continue;
        const unsigned bit = 1u << (w & 31);
        if (atomicOr(&bits[w >> 5], bit) & bit) continue;          // (a word a longer context, or a repeat of this list, has taken)
        nm_patch(yrow, w, base, add + lp);
    }
}

template <int SELF_NORM>
__global__ void __launch_bounds__(NM_THREADS) ngram_mix_rows_kernel(const NmArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned nm_bits[];        // [(V + 31) / 32]: word w is done
    __shared__ float l_m[NM_WAVES], c_bow[2];
    __shared__ double l_s[NM_WAVES];
    __shared__ int c_rng[4];
    const int r = blockIdx.x, tid = threadIdx.x;
    const int live = min(a.n_dev ? *a.n_dev : a.n_rows, a.n_rows);
    if (r >= live) return;                                         // (block-uniform, as every return below)
    int u = a.hist[2 * (size_t)r], v = a.hist[2 * (size_t)r + 1];
    if (u < -1 || u >= a.V || v < -1 || v >= a.V) {
        if (tid == 0 && a.flags) atomicOr(a.flags, 4);
        return;
    }
    if (a.order < 2) v = -1;
    if (a.order < 3 || v < 0) u = -1;

    if (tid == 0) {                                                // the row's contexts
        int b0 = 0, b1 = 0, t0 = 0, t1 = 0;
        float w1 = 0.0f, w2 = 0.0f;
        if (v >= 0) {
            w1 = a.t.uni_bow[v];
            b0 = a.t.bi_off[v];
            b1 = a.t.bi_off[v + 1];
            const int c = u >= 0 ? nm_context(a.t, u, v) : -1;     // (its first trip beside the three loads above)
            if (!(b0 >= 0 && b0 <= b1 && b1 <= a.t.n_bi)) b0 = b1 = 0;
            if (c >= 0 && c < a.t.n_ctx) {
                t0 = a.t.tri_off[c];
                t1 = a.t.tri_off[c + 1];
                w2 = a.t.tri_bow[c];
                if (!(t0 >= 0 && t0 <= t1 && t1 <= a.t.n_tri)) t0 = t1 = 0;
            }
        }
        c_rng[0] = t0; c_rng[1] = t1; c_rng[2] = b0; c_rng[3] = b1;
        c_bow[0] = w2; c_bow[1] = w1;
    }
    for (int i = tid; i < (a.V + 31) >> 5; i += NM_THREADS) nm_bits[i] = 0u;

    float *yrow = a.y + (size_t)r * a.ld_y;
    float L = 0.0f;
    if (!SELF_NORM) {
        float M;
        double S;
        rl_row(reinterpret_cast<const f32x4 *>(yrow), a.V, l_m, l_s, M, S);
        if (!(M > -INFINITY && M < INFINITY && S > 0.0 && S < INFINITY)) {
            if (tid == 0 && a.flags) atomicOr(a.flags, 2);
            return;
        }
        L = (float)((double)M + log(S));
    } else {
        __syncthreads();
    }
    const float base = L + a.log_rho;
    const float w2 = c_bow[0], w1 = c_bow[1];

    nm_list(a.t.tri_w, a.t.tri_lp, c_rng[0], c_rng[1], a.V, nm_bits, yrow, base, 0.0f);
    __syncthreads();
    nm_list(a.t.bi_w, a.t.bi_lp, c_rng[2], c_rng[3], a.V, nm_bits, yrow, base, w2);
    __syncthreads();
    // every remaining word: NM_DEPTH words a thread a trip, their logits and unigrams requested together before any is patched (a
    // row has one workgroup: without that the trips of a wave are one round trip after another)
    const float back = w2 + w1;
    for (int w0 = tid; w0 < a.V; w0 += NM_THREADS * NM_DEPTH) {
        float yw[NM_DEPTH], lp[NM_DEPTH];
#pragma unroll
        for (int k = 0; k < NM_DEPTH; ++k) {
            const int w = w0 + k * NM_THREADS;
            const bool todo = w < a.V && !((nm_bits[w >> 5] >> (w & 31)) & 1u);
            lp[k] = todo ? a.t.uni_lp[w] : -INFINITY;
            yw[k] = todo ? yrow[w] : 0.0f;
        }
#pragma unroll
        for (int k = 0; k < NM_DEPTH; ++k) {
            float out;
            if (lp[k] > -INFINITY && nm_mix(yw[k], base + (back + lp[k]), out)) yrow[w0 + k * NM_THREADS] = out;
        }
    }
}

__global__ void __launch_bounds__(NM_THREADS) ngram_hist_advance_kernel(const int2 *__restrict__ hist_in, int n_in,
                                                                        const int *__restrict__ prev_row, const int *__restrict__ word, int n,
                                                                        int2 *__restrict__ hist_out) {
    const int q = blockIdx.x * NM_THREADS + threadIdx.x;
    if (q >= n) return;
    const int p = prev_row[q];
    const int v = p >= 0 && p < n_in ? hist_in[p].y : -1;
    hist_out[q] = make_int2(v, word[q]);
}

}  // namespace

// the refusals of jlm_ngram_mix_rows on their own (jlm_rank_ngram_frames asks before its first launch): -1, or 0
int jlm_ngram_mix_refuse(const float *y, int ld_y, int n_cols, const jlm_ngram_rows *t, const int *hist, int n_rows, const int *n_dev,
                         float lam, int order, const int *flags) {
    if (!t || order < 1 || order > 3 || !(lam > 0.0f && lam < 1.0f)) return -1;
    if (n_cols < 1 || n_cols > JLM_NGRAM_MIX_MAX_V || ld_y % 4 != 0 || ld_y < ((n_cols + 3) & ~3)) return -1;
    if (n_rows < 0 || t->n_bi < 0 || t->n_tri < 0 || t->n_ctx < 0) return -1;
    if (t->log2cap < 6 || t->log2cap > 31 || t->max_probe < 0 || (long long)t->max_probe >= (1ll << t->log2cap)) return -1;
    if (!t->uni_lp || !t->uni_bow || !t->bi_off || !t->bi_w || !t->bi_lp || !t->tri_off || !t->tri_w || !t->tri_lp || !t->tri_bow ||
        !t->ctx_keys || !t->ctx_vals)
        return -1;
    if ((((uintptr_t)t->uni_lp | (uintptr_t)t->uni_bow | (uintptr_t)t->bi_off | (uintptr_t)t->bi_w | (uintptr_t)t->bi_lp |
          (uintptr_t)t->tri_off | (uintptr_t)t->tri_w | (uintptr_t)t->tri_lp | (uintptr_t)t->tri_bow | (uintptr_t)t->ctx_vals |
          (uintptr_t)hist | (uintptr_t)n_dev | (uintptr_t)flags) & 3) != 0 || ((uintptr_t)t->ctx_keys & 7) != 0)
        return -1;
    if (n_rows == 0) return 0;
    if (!y || !hist || ((uintptr_t)y & 15) != 0) return -1;
    return 0;
}

extern "C" int jlm_ngram_mix_rows(float *y, int ld_y, int n_cols, int self_norm, const jlm_ngram_rows *t, const int *hist, int n_rows,
                                  const int *n_dev, float lam, int order, int *flags, void *stream) {
    if (int rc = jlm_ngram_mix_refuse(y, ld_y, n_cols, t, hist, n_rows, n_dev, lam, order, flags)) return rc;
    if (n_rows == 0) return 0;
    NmArgs a;
    a.y = y; a.t = *t; a.hist = hist; a.n_dev = n_dev; a.flags = flags; a.ld_y = ld_y; a.V = n_cols; a.n_rows = n_rows; a.order = order;
    a.log_rho = (float)(log((double)lam) - log1p(-(double)lam));
    // the bitmap: 48 KB at most (JLM_NGRAM_MIX_MAX_V); the kernel's static LDS (l_m, l_s, c_rng, c_bow: under 100 bytes) comes on top,
    // inside the 64 KB a workgroup may ask for without an attribute
    const size_t lds = (size_t)4 * ((n_cols + 31) >> 5);
    if (self_norm)
        ngram_mix_rows_kernel<1><<<dim3(n_rows), dim3(NM_THREADS), lds, (hipStream_t)stream>>>(a);
    else
        ngram_mix_rows_kernel<0><<<dim3(n_rows), dim3(NM_THREADS), lds, (hipStream_t)stream>>>(a);
    return (int)hipGetLastError();
}

extern "C" int jlm_ngram_hist_advance(const int *hist_in, int n_in, const int *prev_row, const int *word, int n, int *hist_out,
                                      void *stream) {
    if (n < 0 || n_in < 0) return -1;
    if (n == 0) return 0;
    if (!hist_in || !prev_row || !word || !hist_out || hist_in == hist_out) return -1;
    if ((((uintptr_t)hist_in | (uintptr_t)hist_out) & 7) != 0 || (((uintptr_t)prev_row | (uintptr_t)word) & 3) != 0) return -1;
    ngram_hist_advance_kernel<<<dim3((n + NM_THREADS - 1) / NM_THREADS), dim3(NM_THREADS), 0, (hipStream_t)stream>>>(
        (const int2 *)hist_in, n_in, prev_row, word, n, (int2 *)hist_out);
    return (int)hipGetLastError();
}
