// jlm_train.hip -- the kernels of one training step of the LSTM language model (jlm_amd/train.py DeviceStepper).
// The graph is the reference's train/model.py RNNLM_Model; jlm_amd/train.py ReferenceStepper restates it in float64 and is what these
// kernels are judged against.  Every sum has ONE writer and a fixed order (no float atomics): a step gives the same bits run after run.
//
// train_gemm_kernel     C (+)= A B (+ bias) over operands given by element strides: the NT form (both K-contiguous), the row-contracting
//                       TN form (dW = X^T dZ, dEmb = dY^T P) and the NN form (dP += dY Emb).  64 x 64 tile, 4 x 4 per lane, an exact f32
//                       fmaf chain in k order per output element; the k tile sits in LDS once and is read along either axis.
// train_gemm_splitk_kernel, train_gemm_combine_kernel
//                       the same product split over the contraction, the splits' tiles added in order by a second launch (section 23).
// embed_rows_kernel     x = mask (.) Emb[id]: the step's input rows.
// cell_fwd_kernel       z -> i, f, o, g (kept, in place), c, h, and the dropped output r = mask (.) h.
// cell_bwd_kernel       dh = mask (.) dr + dh_next, dc -> dz [B, 4H], dc_prev.
// lse_update_kernel     one wave per row: the chunk's (max, sum exp), granule of 64 words by granule, merged into the row's running pair.
// dy_kernel             logits of a chunk -> dy = s (p (1 + 2 nw lse) - onehot) in place; the target's logit is met on the way.
// colsum_kernel         out[c] (+)= sum over rows in row order (db2 of a chunk, the gate biases).
// ce_kernel             one workgroup: ce = mean(lse - y[target]) in f64 -> the pass's loss slot; a non-finite loss raises the flag word.
// distill_lse_update_kernel, distill_dy_kernel, distill_kl_kernel
//                       the same two passes over a student's and a frozen teacher's logits: three running
//                       normalisers, dy with the soft term, and the Kullback-Leibler row sums, one writer and a fixed order.
// scatter_rows_kernel   dEmb[w] += sum of mask (.) dx over the rows that read word w: the ids sorted, one wave per distinct word, index order.
// adam_kernel           TensorFlow's Adam over the flat parameter buffer, 16-byte accesses; a raised flag word stops every update.
// dyneval_sqacc_kernel, dyneval_rms_kernel, dyneval_mean_kernel, dyneval_update_kernel
//                       dynamic evaluation: ms += g^2, rms = sqrt(ms / chunks) with its f64 mean in a fixed order, and
//                       the decay-to-prior update over the flat parameter buffer.
// expand_codes_kernel   w = book[gid]: the weights of a compressed model from its codebooks (fine-tuning).
// codebook_partial_kernel, codebook_combine_kernel
//                       the codebook gradient: per code the sum of its elements' weight gradients, in f64, a fixed order, one writer.
//
// The dropout mask is a pure function of (key, element): element = row * width + column of the [N, width] array in time-major row order,
// keep <=> splitmix64(key + G (element + 1)) >> 40 < thr, thr = ceil(keep 2^24); key = splitmix64 of (seed, step, site) from the host.
#include "jlm_common.h"

#include <math.h>

typedef unsigned long long u64;
typedef int i32x4 __attribute__((ext_vector_type(4)));

#define TG_BM 64
#define TG_BN 64
#define TG_BK 16
#define TG_LD (TG_BM + 4)

__device__ __forceinline__ bool tr_keep(u64 key, u64 elem, unsigned thr) {
    u64 z = key + 0x9E3779B97F4A7C15ull * (elem + 1ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (unsigned)(z >> 40) < thr;
}

__global__ __launch_bounds__(256) void train_gemm_kernel(const float *__restrict__ A, long long sam, long long sak,
                                                         const float *__restrict__ B, long long sbk, long long sbn, float *C, long long ldc,
                                                         int M, int N, int K, int accumulate, const float *__restrict__ bias, int a_kfast,
                                                         int b_nfast) {
    __shared__ __attribute__((aligned(16))) float As[TG_BK][TG_LD];
    __shared__ __attribute__((aligned(16))) float Bs[TG_BK][TG_LD];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int m0 = blockIdx.y * TG_BM, n0 = blockIdx.x * TG_BN;
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.0f;
    for (int k0 = 0; k0 < K; k0 += TG_BK) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = tid + i * 256;
            int mm, kk;
            if (a_kfast) { kk = idx & 15; mm = idx >> 4; } else { mm = idx & 63; kk = idx >> 6; }
            const int gm = m0 + mm, gk = k0 + kk;
            As[kk][mm] = (gm < M && gk < K) ? A[(long long)gm * sam + (long long)gk * sak] : 0.0f;
            int nn;
            if (b_nfast) { nn = idx & 63; kk = idx >> 6; } else { kk = idx & 15; nn = idx >> 4; }
            const int gn = n0 + nn, gk2 = k0 + kk;
            Bs[kk][nn] = (gn < N && gk2 < K) ? B[(long long)gk2 * sbk + (long long)gn * sbn] : 0.0f;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < TG_BK; ++kk) {
            const f32x4 a = *reinterpret_cast<const f32x4 *>(&As[kk][ty * 4]);
            const f32x4 b = *reinterpret_cast<const f32x4 *>(&Bs[kk][tx * 4]);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(a[i], b[j], acc[i][j]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int gm = m0 + ty * 4 + i;
        if (gm >= M) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int gn = n0 + tx * 4 + j;
            if (gn >= N) continue;
            float v = acc[i][j];
            if (bias) v += bias[gn];
            float *c = C + (long long)gm * ldc + gn;
            if (accumulate) v += *c;
            *c = v;
        }
    }
}

extern "C" int jlm_train_gemm(const float *A, long long sam, long long sak, const float *B, long long sbk, long long sbn, float *C, int ldc,
                              int M, int N, int K, int accumulate, const float *bias, void *stream) {
    if (!A || !B || !C || M < 1 || N < 1 || K < 1 || ldc < N || sam < 1 || sak < 1 || sbk < 1 || sbn < 1) return -1;
    const long long gy = (M + TG_BM - 1) / TG_BM, gx = (N + TG_BN - 1) / TG_BN;
    if (gy > 65535 || gx > 2147483647ll) return -1;
    hipLaunchKernelGGL(train_gemm_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, (hipStream_t)stream, A, sam, sak, B, sbk, sbn, C,
                       (long long)ldc, M, N, K, accumulate, bias, sak == 1 ? 1 : 0, sbn == 1 ? 1 : 0);
    JLM_LAUNCH_CHECK();
    return 0;
}

// The same product split over the contraction: at B T of a few rows C has a handful of tiles under a K as long as
// the vocabulary.  Split s = blockIdx.z runs the fmaf chain over [s kc, min(K, (s + 1) kc)) and writes its tile to part[s][M][N];
// train_gemm_combine_kernel then forms v = part[0] + part[1] + ... in that order, adds the bias, then *c when accumulating -- the
// epilogue order above.  One writer per element and no atomics: the bits depend on the operands and kc alone, and one split gives
// train_gemm_kernel's.
// train_gemm_kernel's tile loop over the k tiles of [k_lo, k_hi) (k_lo a multiple of TG_BK): the same loads, the same fmaf chain per output
// element in k order.  (A copy, not a shared function: the trainer's kernel stays the code it was.)
__device__ __forceinline__ void tg_accumulate(const float *__restrict__ A, long long sam, long long sak, const float *__restrict__ B,
                                              long long sbk, long long sbn, int M, int N, int k_lo, int k_hi, int a_kfast, int b_nfast,
                                              float (&acc)[4][4]) {
    __shared__ __attribute__((aligned(16))) float As[TG_BK][TG_LD];
    __shared__ __attribute__((aligned(16))) float Bs[TG_BK][TG_LD];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int m0 = blockIdx.y * TG_BM, n0 = blockIdx.x * TG_BN;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.0f;
    for (int k0 = k_lo; k0 < k_hi; k0 += TG_BK) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = tid + i * 256;
            int mm, kk;
            if (a_kfast) { kk = idx & 15; mm = idx >> 4; } else { mm = idx & 63; kk = idx >> 6; }
            const int gm = m0 + mm, gk = k0 + kk;
            As[kk][mm] = (gm < M && gk < k_hi) ? A[(long long)gm * sam + (long long)gk * sak] : 0.0f;
            int nn;
            if (b_nfast) { nn = idx & 63; kk = idx >> 6; } else { kk = idx & 15; nn = idx >> 4; }
            const int gn = n0 + nn, gk2 = k0 + kk;
            Bs[kk][nn] = (gn < N && gk2 < k_hi) ? B[(long long)gk2 * sbk + (long long)gn * sbn] : 0.0f;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < TG_BK; ++kk) {
            const f32x4 a = *reinterpret_cast<const f32x4 *>(&As[kk][ty * 4]);
            const f32x4 b = *reinterpret_cast<const f32x4 *>(&Bs[kk][tx * 4]);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(a[i], b[j], acc[i][j]);
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void train_gemm_splitk_kernel(const float *__restrict__ A, long long sam, long long sak,
                                                                const float *__restrict__ B, long long sbk, long long sbn,
                                                                float *__restrict__ part, int M, int N, int K, int kc, int a_kfast,
                                                                int b_nfast) {
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int m0 = blockIdx.y * TG_BM, n0 = blockIdx.x * TG_BN;
    const long long k_lo = (long long)blockIdx.z * kc;
    const int k_hi = (int)(k_lo + kc < K ? k_lo + kc : K);
    float acc[4][4];
    tg_accumulate(A, sam, sak, B, sbk, sbn, M, N, (int)k_lo, k_hi, a_kfast, b_nfast, acc);
    float *out = part + (long long)blockIdx.z * M * N;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int gm = m0 + ty * 4 + i;
        if (gm >= M) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int gn = n0 + tx * 4 + j;
            if (gn < N) out[(long long)gm * N + gn] = acc[i][j];
        }
    }
}

__global__ __launch_bounds__(256) void train_gemm_combine_kernel(const float *__restrict__ part, int n_split, float *C, long long ldc, int M,
                                                                 int N, int accumulate, const float *__restrict__ bias) {
    const long long mn = (long long)M * N, e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= mn) return;
    const int gm = (int)(e / N), gn = (int)(e % N);
    float v = part[e];
    for (int s = 1; s < n_split; ++s) v += part[s * mn + e];
    if (bias) v += bias[gn];
    float *c = C + (long long)gm * ldc + gn;
    if (accumulate) v += *c;
    *c = v;
}

extern "C" int jlm_train_gemm_splitk(const float *A, long long sam, long long sak, const float *B, long long sbk, long long sbn, float *C,
                                     int ldc, int M, int N, int K, int accumulate, const float *bias, int kc, float *part,
                                     long long part_elems, void *stream) {
    if (!A || !B || !C || !part || M < 1 || N < 1 || K < 1 || ldc < N || sam < 1 || sak < 1 || sbk < 1 || sbn < 1) return -1;
    if (kc < TG_BK || kc % TG_BK) return -1;
    const long long gy = (M + TG_BM - 1) / TG_BM, gx = (N + TG_BN - 1) / TG_BN, gz = ((long long)K + kc - 1) / kc, mn = (long long)M * N;
    if (gy > 65535 || gz > 65535 || gx > 2147483647ll || part_elems < gz * mn || (mn + 255) / 256 > 2147483647ll) return -1;
    hipLaunchKernelGGL(train_gemm_splitk_kernel, dim3((unsigned)gx, (unsigned)gy, (unsigned)gz), dim3(256), 0, (hipStream_t)stream, A, sam,
                       sak, B, sbk, sbn, part, M, N, K, kc, sak == 1 ? 1 : 0, sbn == 1 ? 1 : 0);
    JLM_LAUNCH_CHECK();
    hipLaunchKernelGGL(train_gemm_combine_kernel, dim3((unsigned)((mn + 255) / 256)), dim3(256), 0, (hipStream_t)stream, part, (int)gz, C,
                       (long long)ldc, M, N, accumulate, bias);
    JLM_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------- input rows
__global__ __launch_bounds__(256) void embed_rows_kernel(const float *__restrict__ emb, int ld_emb, int V, const int *__restrict__ ids,
                                                         int n_rows, int E, float *__restrict__ x, u64 key, unsigned thr, float scale) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)n_rows * E) return;
    const int r = (int)(i / E), e = (int)(i % E);
    const int w = ids[r];
    float v = 0.0f;
    if (w >= 0 && w < V && tr_keep(key, (u64)i, thr)) v = emb[(long long)w * ld_emb + e] * scale;
    x[i] = v;
}

extern "C" int jlm_train_embed_rows(const float *emb, int ld_emb, int V, const int *ids, int n_rows, int E, float *x, uint64_t key,
                                    unsigned thr, float scale, void *stream) {
    if (!emb || !ids || !x || n_rows < 1 || E < 1 || ld_emb < E || V < 1) return -1;
    const long long n = (long long)n_rows * E;
    hipLaunchKernelGGL(embed_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, emb, ld_emb, V, ids, n_rows,
                       E, x, (u64)key, thr, scale);
    JLM_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------- the LSTM cell
__device__ __forceinline__ float tr_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// z [B, 4H] (i | f | o | g pre-activations) -> the activations in place; c, h [B, H]; r = mask (.) h.  row0: the step's first row in the
// [N, H] time-major array the mask is defined over.
__global__ __launch_bounds__(256) void cell_fwd_kernel(float *__restrict__ z, const float *__restrict__ c_prev, float *__restrict__ c,
                                                       float *__restrict__ h, float *__restrict__ r, int B, int H, long long row0, u64 key,
                                                       unsigned thr, float scale) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= B * H) return;
    const int b = idx / H, j = idx % H;
    float *zr = z + (long long)b * 4 * H;
    const float gi = tr_sigmoid(zr[j]), gf = tr_sigmoid(zr[H + j]), go = tr_sigmoid(zr[2 * H + j]), gg = tanhf(zr[3 * H + j]);
    zr[j] = gi; zr[H + j] = gf; zr[2 * H + j] = go; zr[3 * H + j] = gg;
    const float cc = fmaf(c_prev[idx], gf, gg * gi);
    const float hh = tanhf(cc) * go;
    c[idx] = cc;
    h[idx] = hh;
    r[idx] = tr_keep(key, (u64)(row0 * H) + (u64)idx, thr) ? hh * scale : 0.0f;
}

extern "C" int jlm_train_cell_fwd(float *z, const float *c_prev, float *c, float *h, float *r, int B, int H, long long row0, uint64_t key,
                                  unsigned thr, float scale, void *stream) {
    if (!z || !c_prev || !c || !h || !r || B < 1 || H < 1 || row0 < 0 || (long long)B * H > 2147483647ll) return -1;
    hipLaunchKernelGGL(cell_fwd_kernel, dim3((unsigned)((B * H + 255) / 256)), dim3(256), 0, (hipStream_t)stream, z, c_prev, c, h, r, B, H,
                       row0, (u64)key, thr, scale);
    JLM_LAUNCH_CHECK();
    return 0;
}

// gates [B, 4H] (activations), c, c_prev [B, H]; dr [B, H]: the gradient of the dropped output; dh_next [B, H] or NULL; dc [B, H] in / out
// (NULL-free: the caller zeroes it before the last step); dz [B, 4H] out.
__global__ __launch_bounds__(256) void cell_bwd_kernel(const float *__restrict__ gates, const float *__restrict__ c,
                                                       const float *__restrict__ c_prev, const float *__restrict__ dr,
                                                       const float *__restrict__ dh_next, float *__restrict__ dc, float *__restrict__ dz,
                                                       int B, int H, long long row0, u64 key, unsigned thr, float scale) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= B * H) return;
    const int b = idx / H, j = idx % H;
    const float *g = gates + (long long)b * 4 * H;
    const float gi = g[j], gf = g[H + j], go = g[2 * H + j], gg = g[3 * H + j];
    float dh = tr_keep(key, (u64)(row0 * H) + (u64)idx, thr) ? dr[idx] * scale : 0.0f;
    if (dh_next) dh += dh_next[idx];
    const float tc = tanhf(c[idx]);
    const float dcc = dc[idx] + dh * go * (1.0f - tc * tc);
    float *d = dz + (long long)b * 4 * H;
    d[j] = dcc * gg * gi * (1.0f - gi);
    d[H + j] = dcc * c_prev[idx] * gf * (1.0f - gf);
    d[2 * H + j] = dh * tc * go * (1.0f - go);
    d[3 * H + j] = dcc * gi * (1.0f - gg * gg);
    dc[idx] = dcc * gf;
}

extern "C" int jlm_train_cell_bwd(const float *gates, const float *c, const float *c_prev, const float *dr, const float *dh_next, float *dc,
                                  float *dz, int B, int H, long long row0, uint64_t key, unsigned thr, float scale, void *stream) {
    if (!gates || !c || !c_prev || !dr || !dc || !dz || B < 1 || H < 1 || row0 < 0 || (long long)B * H > 2147483647ll) return -1;
    hipLaunchKernelGGL(cell_bwd_kernel, dim3((unsigned)((B * H + 255) / 256)), dim3(256), 0, (hipStream_t)stream, gates, c, c_prev, dr,
                       dh_next, dc, dz, B, H, row0, (u64)key, thr, scale);
    JLM_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------- the vocabulary loss
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// The chunk is met in granules of 64 words from its first: a granule's (max, sum exp) comes from one value per lane through the xor
// butterflies and is merged into the row's running pair, granules in order.  A chunk that starts at a multiple of 64 words of the
// vocabulary (DeviceStepper's windows do) therefore leaves the same bits as any other cut of the same words into such chunks.
__global__ __launch_bounds__(256) void lse_update_kernel(const float *__restrict__ y, long long ld, int n_cols, int n_rows,
                                                         float *__restrict__ run_m, float *__restrict__ run_s, int first) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n_rows) return;
    const float *yr = y + (long long)row * ld;
    float M0 = JLM_NEG_BIG, S0 = 0.0f;                     // every lane carries the pair: the butterflies leave all lanes the same bits
    if (!first) { M0 = run_m[row]; S0 = run_s[row]; }
    for (int c0 = 0; c0 < n_cols; c0 += 64) {
        const int c = c0 + lane;
        const float v = c < n_cols ? yr[c] : JLM_NEG_BIG;
        const float m = wave_max(v);
        const float s = wave_sum(c < n_cols ? expf(v - m) : 0.0f);
        lse_merge(M0, S0, m, s);
    }
    if (lane == 0) {
        run_m[row] = M0;
        run_s[row] = S0;
    }
}

extern "C" int jlm_train_lse_update(const float *y, int ld, int n_cols, int n_rows, float *run_m, float *run_s, int first, void *stream) {
    if (!y || !run_m || !run_s || n_cols < 1 || n_rows < 1 || ld < n_cols) return -1;
    hipLaunchKernelGGL(lse_update_kernel, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, y, (long long)ld, n_cols,
                       n_rows, run_m, run_s, first);
    JLM_LAUNCH_CHECK();
    return 0;
}

// y [n_rows, ld]: the logits of words [v0, v0 + n_cols) -> dy in place.  s = 1 / N; nw2 = 2 norm_weight (0: no self-normalisation term).
__global__ __launch_bounds__(256) void dy_kernel(float *__restrict__ y, long long ld, int n_cols, int v0, int n_rows,
                                                 const float *__restrict__ run_m, const float *__restrict__ run_s,
                                                 const int *__restrict__ target, float *__restrict__ tgt_logit, float s, float nw2) {
    const int row = blockIdx.y;
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (row >= n_rows || c >= n_cols) return;
    const float lse = run_m[row] + logf(run_s[row]);
    float *p = y + (long long)row * ld + c;
    const float v = *p;
    const bool hit = target[row] == v0 + c;
    if (hit) tgt_logit[row] = v;
    const float pr = expf(v - lse);
    *p = s * (fmaf(pr * nw2, lse, pr) - (hit ? 1.0f : 0.0f));
}

extern "C" int jlm_train_dy(float *y, int ld, int n_cols, int v0, int n_rows, const float *run_m, const float *run_s, const int *target,
                            float *tgt_logit, float s, float nw2, void *stream) {
    if (!y || !run_m || !run_s || !target || !tgt_logit || n_cols < 1 || n_rows < 1 || n_rows > 65535 || ld < n_cols || v0 < 0) return -1;
    hipLaunchKernelGGL(dy_kernel, dim3((unsigned)((n_cols + 255) / 256), (unsigned)n_rows), dim3(256), 0, (hipStream_t)stream, y,
                       (long long)ld, n_cols, v0, n_rows, run_m, run_s, target, tgt_logit, s, nw2);
    JLM_LAUNCH_CHECK();
    return 0;
}

__global__ __launch_bounds__(256) void colsum_kernel(const float *__restrict__ a, long long ld, int n_rows, int n_cols, float *__restrict__ out,
                                                     int accumulate) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= n_cols) return;
    float s = 0.0f;
    for (int r = 0; r < n_rows; ++r) s += a[(long long)r * ld + c];
    out[c] = accumulate ? out[c] + s : s;
}

extern "C" int jlm_train_colsum(const float *a, int ld, int n_rows, int n_cols, float *out, int accumulate, void *stream) {
    if (!a || !out || n_rows < 1 || n_cols < 1 || ld < n_cols) return -1;
    hipLaunchKernelGGL(colsum_kernel, dim3((unsigned)((n_cols + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, (long long)ld, n_rows,
                       n_cols, out, accumulate);
    JLM_LAUNCH_CHECK();
    return 0;
}

// nw: norm_weight (0 without self-normalisation).  The training loss is ce + nw mean(lse^2); where that is not finite IN F32 (an lse
// whose square overflows counts) the step is flagged and its slot holds +inf, so that the host can name the step.
__global__ __launch_bounds__(256) void ce_kernel(const float *__restrict__ run_m, const float *__restrict__ run_s,
                                                 const float *__restrict__ tgt_logit, int n_rows, float nw, double *__restrict__ ce_out,
                                                 int *__restrict__ flag) {
    __shared__ double part[256];
    double s = 0.0;
    int bad = 0;
    for (int r = threadIdx.x; r < n_rows; r += 256) {
        const float lse = run_m[r] + logf(run_s[r]);
        s += (double)lse - (double)tgt_logit[r];
        bad |= !isfinite(lse) || (nw != 0.0f && !isfinite(nw * (lse * lse)));
    }
    bad = __syncthreads_or(bad);
    part[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double ce = part[0] / (double)n_rows;
        if (bad || !isfinite(ce) || !isfinite((float)ce)) {
            ce_out[0] = (double)INFINITY;
            flag[0] = 1;
        } else {
            ce_out[0] = ce;
        }
    }
}

extern "C" int jlm_train_ce(const float *run_m, const float *run_s, const float *tgt_logit, int n_rows, float nw, double *ce_out, int *flag,
                            void *stream) {
    if (!run_m || !run_s || !tgt_logit || !ce_out || !flag || n_rows < 1) return -1;
    hipLaunchKernelGGL(ce_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, run_m, run_s, tgt_logit, n_rows, nw, ce_out, flag);
    JLM_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------- the distillation loss
// A student's logits y_s and a frozen teacher's y_t over the same words (jlm_amd/distill.py).  run [6, n_rows]
// holds three running (max, sum exp) pairs: rows 0, 1 of y_s (L_s), rows 2, 3 of y_s / tau (A_s), rows 4, 5 of y_t / tau (A_t).
//
// Pass 1 walks the window as lse_update_kernel does, each logit read once: granules of 64 words from the window's first, one value per
// lane, xor butterflies, merged in order.  Windows that start on multiples of 64 words leave the same bits however the words are cut,
// and at inv_tau == 1.0f (y * 1.0f is y) the L_s pair is lse_update_kernel's and the A_s pair is the L_s pair, bit for bit.
__global__ __launch_bounds__(256) void distill_lse_update_kernel(const float *__restrict__ ys, long long ld_s, const float *__restrict__ yt,
                                                                 long long ld_t, int n_cols, int n_rows, float inv_tau,
                                                                 float *__restrict__ run, int first) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n_rows) return;
    const float *sr = ys + (long long)row * ld_s, *tr = yt + (long long)row * ld_t;
    float M[3] = {JLM_NEG_BIG, JLM_NEG_BIG, JLM_NEG_BIG}, S[3] = {0.0f, 0.0f, 0.0f};
    if (!first) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            M[k] = run[(long long)(2 * k) * n_rows + row];
            S[k] = run[(long long)(2 * k + 1) * n_rows + row];
        }
    }
    for (int c0 = 0; c0 < n_cols; c0 += 64) {
        const int c = c0 + lane;
        const bool in = c < n_cols;
        float v[3] = {JLM_NEG_BIG, JLM_NEG_BIG, JLM_NEG_BIG};
        if (in) {
            v[0] = sr[c];
            v[1] = v[0] * inv_tau;
            v[2] = tr[c] * inv_tau;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float m = wave_max(v[k]);
            const float s = wave_sum(in ? expf(v[k] - m) : 0.0f);
            lse_merge(M[k], S[k], m, s);
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            run[(long long)(2 * k) * n_rows + row] = M[k];
            run[(long long)(2 * k + 1) * n_rows + row] = S[k];
        }
    }
}

extern "C" int jlm_distill_lse_update(const float *ys, int ld_s, const float *yt, int ld_t, int n_cols, int n_rows, float inv_tau, float *run,
                                      int first, void *stream) {
    if (!ys || !yt || !run || n_cols < 1 || n_rows < 1 || ld_s < n_cols || ld_t < n_cols || !(inv_tau > 0.0f) || !isfinite(inv_tau))
        return -1;
    hipLaunchKernelGGL(distill_lse_update_kernel, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, ys,
                       (long long)ld_s, yt, (long long)ld_t, n_cols, n_rows, inv_tau, run, first);
    JLM_LAUNCH_CHECK();
    return 0;
}

// Pass 2, one wave per row over the window's granules in order.  With p = exp(y_s - L_s), p^tau = exp(y_s / tau - A_s) and
// q = exp(y_t / tau - A_t):  dy = s (c_hard (p - onehot) + nw2 L_s p + c_soft (p^tau - q)) in place over y_s, with c_hard = 1 - alpha and
// c_soft = alpha tau from the host; the target's logit is met on the way.  The row's Kullback-Leibler terms q (log q - log p^tau), in
// log space (q == 0 adds 0; a q that is not a number stays one), are added by butterfly per granule and the granule sums taken in order
// into kl_row[row], which this wave alone writes and which starts at 0 when `first` is set: kl_row does not depend on the cut either.
__global__ __launch_bounds__(256) void distill_dy_kernel(float *__restrict__ ys, long long ld_s, const float *__restrict__ yt, long long ld_t,
                                                         int n_cols, int v0, int n_rows, const float *__restrict__ run,
                                                         const int *__restrict__ target, float *__restrict__ tgt_logit,
                                                         float *__restrict__ kl_row, float s, float nw2, float c_hard, float c_soft,
                                                         float inv_tau, int first) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n_rows) return;
    float *sr = ys + (long long)row * ld_s;
    const float *tr = yt + (long long)row * ld_t;
    const float Ls = run[row] + logf(run[(long long)n_rows + row]);
    const float As = run[2ll * n_rows + row] + logf(run[3ll * n_rows + row]);
    const float At = run[4ll * n_rows + row] + logf(run[5ll * n_rows + row]);
    const int tg = target[row] - v0;
    float kl = first ? 0.0f : kl_row[row];
    for (int c0 = 0; c0 < n_cols; c0 += 64) {
        const int c = c0 + lane;
        float term = 0.0f;
        if (c < n_cols) {
            const float vs = sr[c], vt = tr[c];
            const bool hit = c == tg;
            if (hit) tgt_logit[row] = vs;
            const float ls = vs * inv_tau - As, lt = vt * inv_tau - At;
            const float p = expf(vs - Ls), pt = expf(ls), q = expf(lt);
            term = q == 0.0f ? 0.0f : q * (lt - ls);
            sr[c] = s * (c_hard * (p - (hit ? 1.0f : 0.0f)) + (p * nw2) * Ls + c_soft * (pt - q));
        }
        kl += wave_sum(term);
    }
    if (lane == 0) kl_row[row] = kl;
}

extern "C" int jlm_distill_dy(float *ys, int ld_s, const float *yt, int ld_t, int n_cols, int v0, int n_rows, const float *run,
                              const int *target, float *tgt_logit, float *kl_row, float s, float nw2, float c_hard, float c_soft,
                              float inv_tau, int first, void *stream) {
    if (!ys || !yt || !run || !target || !tgt_logit || !kl_row || n_cols < 1 || n_rows < 1 || ld_s < n_cols || ld_t < n_cols || v0 < 0 ||
        !(inv_tau > 0.0f) || !isfinite(inv_tau))
        return -1;
    hipLaunchKernelGGL(distill_dy_kernel, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, ys, (long long)ld_s, yt,
                       (long long)ld_t, n_cols, v0, n_rows, run, target, tgt_logit, kl_row, s, nw2, c_hard, c_soft, inv_tau, first);
    JLM_LAUNCH_CHECK();
    return 0;
}

// One workgroup, in ce_kernel's shape: kl_out[0] = the mean of kl_row in f64.  A value that is not finite gives +inf and raises the flag
// word that stops Adam.
__global__ __launch_bounds__(256) void distill_kl_kernel(const float *__restrict__ kl_row, int n_rows, double *__restrict__ kl_out,
                                                         int *__restrict__ flag) {
    __shared__ double part[256];
    double s = 0.0;
    int bad = 0;
    for (int r = threadIdx.x; r < n_rows; r += 256) {
        const float k = kl_row[r];
        s += (double)k;
        bad |= !isfinite(k);
    }
    bad = __syncthreads_or(bad);
    part[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double kl = part[0] / (double)n_rows;
        if (bad || !isfinite(kl) || !isfinite((float)kl)) {
            kl_out[0] = (double)INFINITY;
            flag[0] = 1;
        } else {
            kl_out[0] = kl;
        }
    }
}

extern "C" int jlm_distill_kl(const float *kl_row, int n_rows, double *kl_out, int *flag, void *stream) {
    if (!kl_row || !kl_out || !flag || n_rows < 1) return -1;
    hipLaunchKernelGGL(distill_kl_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, kl_row, n_rows, kl_out, flag);
    JLM_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------- the input side of dEmb
// ids_sorted [n]: the step's input ids ascending; perm [n]: the row each came from (a stable sort: rows ascending within a word).
// One wave per position that opens a run of equal ids; it adds the run's rows in index order and adds the sum to the word's row of the
// target, which nobody else writes in this launch.  The target holds the words [v_lo, v_hi) and columns [col0, col0 + n_cols) of the
// [V, width] gradient (a D_softmax block, LM0 of a V_table model, or everything); words outside the range are left alone.
__global__ __launch_bounds__(256) void scatter_rows_kernel(const float *__restrict__ dx, int ld_dx, int col0, int n_cols, int width,
                                                           const int *__restrict__ ids_sorted, const long long *__restrict__ perm, int n,
                                                           float *__restrict__ demb, int ld, int v_lo, int v_hi, u64 key, unsigned thr,
                                                           float scale) {
    const int pos = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (pos >= n) return;
    const int w = ids_sorted[pos];
    if (w < v_lo || w >= v_hi || (pos > 0 && ids_sorted[pos - 1] == w)) return;
    for (int e = lane; e < n_cols; e += 64) {
        float s = 0.0f;
        for (int q = pos; q < n && ids_sorted[q] == w; ++q) {
            const long long r = perm[q];
            if (r < 0 || r >= n) continue;
            if (tr_keep(key, (u64)r * (u64)width + (u64)(col0 + e), thr)) s += dx[r * ld_dx + col0 + e] * scale;
        }
        demb[(long long)(w - v_lo) * ld + e] += s;
    }
}

extern "C" int jlm_train_scatter_rows(const float *dx, int ld_dx, int col0, int n_cols, int width, const int *ids_sorted,
                                      const long long *perm, int n, float *demb, int ld, int v_lo, int v_hi, uint64_t key, unsigned thr,
                                      float scale, void *stream) {
    if (!dx || !ids_sorted || !perm || !demb || n < 1 || n_cols < 1 || col0 < 0 || col0 + n_cols > width || ld_dx < width || ld < n_cols ||
        v_lo < 0 || v_hi <= v_lo)
        return -1;
    hipLaunchKernelGGL(scatter_rows_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, dx, ld_dx, col0, n_cols, width,
                       ids_sorted, perm, n, demb, ld, v_lo, v_hi, (u64)key, thr, scale);
    JLM_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------- Adam
// TensorFlow's form: m <- b1 m + (1 - b1) g; v <- b2 v + (1 - b2) g^2; w <- w - lr_t m / (sqrt(v) + eps); lr_t from the host.
__device__ __forceinline__ void adam_one(float &w, float g, float &m, float &v, float lr_t) {
    m = fmaf(0.9f, m, 0.1f * g);
    v = fmaf(0.999f, v, 0.001f * (g * g));
    w -= lr_t * m / (sqrtf(v) + 1e-8f);
}

__global__ __launch_bounds__(256) void adam_kernel(float *__restrict__ w, const float *__restrict__ g, float *__restrict__ m,
                                                   float *__restrict__ v, long long n4, float lr_t, const int *__restrict__ flag) {
    if (flag && flag[0]) return;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        f32x4 ww = reinterpret_cast<f32x4 *>(w)[i], mm = reinterpret_cast<f32x4 *>(m)[i], vv = reinterpret_cast<f32x4 *>(v)[i];
        const f32x4 gg = reinterpret_cast<const f32x4 *>(g)[i];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float w1 = ww[k], m1 = mm[k], v1 = vv[k];
            adam_one(w1, gg[k], m1, v1, lr_t);
            ww[k] = w1; mm[k] = m1; vv[k] = v1;
        }
        reinterpret_cast<f32x4 *>(w)[i] = ww;
        reinterpret_cast<f32x4 *>(m)[i] = mm;
        reinterpret_cast<f32x4 *>(v)[i] = vv;
    }
}

// n: a multiple of 4 (the flat parameter buffer pads every tensor to 16 bytes); all four pointers 16-byte aligned
extern "C" int jlm_train_adam(float *w, const float *g, float *m, float *v, long long n, float lr_t, const int *flag, void *stream) {
    if (!w || !g || !m || !v || n < 4 || (n & 3) || ((uintptr_t)w | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) return -1;
    const long long n4 = n / 4;
    long long grid = (n4 + 255) / 256;
    if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(adam_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, w, g, m, v, n4, lr_t, flag);
    JLM_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------- dynamic evaluation
// (jlm_amd/dyneval.py).  All three walk the flat parameter buffer as adam_kernel does: 16-byte accesses, grid-stride.
__global__ __launch_bounds__(256) void dyneval_sqacc_kernel(float *__restrict__ ms, const float *__restrict__ g, long long n4,
                                                            const int *__restrict__ flag) {
    if (flag && flag[0]) return;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        f32x4 mm = reinterpret_cast<f32x4 *>(ms)[i];
        const f32x4 gg = reinterpret_cast<const f32x4 *>(g)[i];
#pragma unroll
        for (int k = 0; k < 4; ++k) mm[k] = fmaf(gg[k], gg[k], mm[k]);
        reinterpret_cast<f32x4 *>(ms)[i] = mm;
    }
}

static long long flat_grid(long long n4) {
    const long long grid = (n4 + 255) / 256;
    return grid > JLM_DYNEVAL_MAX_BLOCKS ? JLM_DYNEVAL_MAX_BLOCKS : grid;
}

extern "C" int jlm_dyneval_sqacc(float *ms, const float *g, long long n, const int *flag, void *stream) {
    if (!ms || !g || n < 4 || (n & 3) || ((uintptr_t)ms | (uintptr_t)g) & 15) return -1;
    hipLaunchKernelGGL(dyneval_sqacc_kernel, dim3((unsigned)flat_grid(n / 4)), dim3(256), 0, (hipStream_t)stream, ms, g, n / 4, flag);
    JLM_LAUNCH_CHECK();
    return 0;
}

// rms = sqrtf(ms inv_chunks), and the f64 sum of those f32 values in a fixed order: a lane adds its elements in the order it meets
// them, the block's 256 lane sums meet in an LDS tree (stride 128, 64, ..., 1), lane 0 writes partial[block].
__global__ __launch_bounds__(256) void dyneval_rms_kernel(const float *__restrict__ ms, long long n4, float inv_chunks,
                                                          float *__restrict__ rms, double *__restrict__ partial) {
    __shared__ double red[256];
    double s = 0.0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const f32x4 mm = reinterpret_cast<const f32x4 *>(ms)[i];
        f32x4 rr;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            rr[k] = sqrtf(mm[k] * inv_chunks);
            s += (double)rr[k];
        }
        reinterpret_cast<f32x4 *>(rms)[i] = rr;
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

// one workgroup: the blocks' sums in index order -> the mean over the n_real parameters (the padding words hold 0 and add nothing)
__global__ __launch_bounds__(64) void dyneval_mean_kernel(const double *__restrict__ partial, int n_partial, long long n_real,
                                                          double *__restrict__ mean_out) {
    if (threadIdx.x) return;
    double s = 0.0;
    for (int b = 0; b < n_partial; ++b) s += partial[b];
    mean_out[0] = s / (double)n_real;
}

extern "C" int jlm_dyneval_rms(const float *ms, long long n, float inv_chunks, float *rms, long long n_real, double *partial,
                               double *mean_out, void *stream) {
    if (!ms || !rms || !partial || !mean_out || n < 4 || (n & 3) || n_real < 1 || n_real > n || !(inv_chunks > 0.0f) ||
        ((uintptr_t)ms | (uintptr_t)rms) & 15)
        return -1;
    const long long grid = flat_grid(n / 4);
    hipLaunchKernelGGL(dyneval_rms_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, ms, n / 4, inv_chunks, rms, partial);
    JLM_LAUNCH_CHECK();
    hipLaunchKernelGGL(dyneval_mean_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, partial, (int)grid, n_real, mean_out);
    JLM_LAUNCH_CHECK();
    return 0;
}

// The decay-to-prior update.  Per element the float64 stepper's expression is evaluated in f64, in its order, and rounded to f32 once:
//   r = rms ? rms[i] : 1;  step = lr g, with rms step = lr g / (r + eps);  c = min(lam_scale r, 1)
//   w = (float)(((double)w - step) + c ((double)w0 - (double)w))
// lam_scale is lambda under the sgd rule and lambda / mean(RMS) under the rms rule.  A padding word (w = g = w0 = rms = 0) stays 0.
// The pass moves 16 or 20 bytes per element, so the f64 arithmetic (one division under the rms rule) hides behind the memory traffic.
__global__ __launch_bounds__(256) void dyneval_update_kernel(float *__restrict__ w, const float *__restrict__ g, const float *__restrict__ w0,
                                                             const float *__restrict__ rms, long long n4, double lr, double lam_scale,
                                                             double eps, const int *__restrict__ flag) {
    if (flag && flag[0]) return;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        f32x4 ww = reinterpret_cast<f32x4 *>(w)[i];
        const f32x4 gg = reinterpret_cast<const f32x4 *>(g)[i], w00 = reinterpret_cast<const f32x4 *>(w0)[i];
        f32x4 rr = {1.0f, 1.0f, 1.0f, 1.0f};
        if (rms) rr = reinterpret_cast<const f32x4 *>(rms)[i];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double wk = (double)ww[k], r = (double)rr[k];
            double step = lr * (double)gg[k];
            if (rms) step = step / (r + eps);
            ww[k] = (float)((wk - step) + fmin(lam_scale * r, 1.0) * ((double)w00[k] - wk));
        }
        reinterpret_cast<f32x4 *>(w)[i] = ww;
    }
}

extern "C" int jlm_dyneval_update(float *w, const float *g, const float *w0, const float *rms, long long n, double lr, double lam_scale,
                                  double eps, const int *flag, void *stream) {
    if (!w || !g || !w0 || n < 4 || (n & 3) || ((uintptr_t)w | (uintptr_t)g | (uintptr_t)w0 | (uintptr_t)rms) & 15) return -1;
    hipLaunchKernelGGL(dyneval_update_kernel, dim3((unsigned)flat_grid(n / 4)), dim3(256), 0, (hipStream_t)stream, w, g, w0, rms, n / 4, lr,
                       lam_scale, eps, flag);
    JLM_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------- codebook fine-tuning
// (jlm_amd/finetune.py).  The weights of a compressed model are w[i] = book[gid[i]]: gid = tensor * K + code for a
// coded element of the flat parameter buffer, -1 for the padding between tensors.
__global__ __launch_bounds__(256) void expand_codes_kernel(const float *__restrict__ book, int n_book, const int *__restrict__ gid,
                                                           float *__restrict__ w, long long n4) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const i32x4 id = reinterpret_cast<const i32x4 *>(gid)[i];
        f32x4 v;
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = (id[k] >= 0 && id[k] < n_book) ? book[id[k]] : 0.0f;
        reinterpret_cast<f32x4 *>(w)[i] = v;
    }
}

extern "C" int jlm_train_expand_codes(const float *book, int n_book, const int *gid, float *w, long long n, void *stream) {
    if (!book || !gid || !w || n_book < 1 || n < 4 || (n & 3) || ((uintptr_t)gid | (uintptr_t)w) & 15) return -1;
    const long long n4 = n / 4;
    long long grid = (n4 + 255) / 256;
    if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(expand_codes_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, book, n_book, gid, w, n4);
    JLM_LAUNCH_CHECK();
    return 0;
}

// The codebook gradient: gbook[j] = sum of g over the elements whose gid is j.  order [n_order]: the offsets of the coded elements sorted
// by (gid, offset); chunks [n_chunks][3] = (group, begin, length): every group's run of `order` cut into pieces of at most
// JLM_CODEBOOK_CHUNK, ascending in group, then in begin.
// First launch: one wave per chunk.  Lane l adds elements l, l + 64, ... of the chunk in that order in f64; the 64 lane sums meet in the
// xor butterfly 32, 16, 8, 4, 2, 1 (f64 addition commutes, so every lane holds the same bits); lane 0 writes the chunk's f64 sum.
__global__ __launch_bounds__(256) void codebook_partial_kernel(const float *__restrict__ g, long long n, const int *__restrict__ order,
                                                               long long n_order, const int *__restrict__ chunks, int n_chunks,
                                                               double *__restrict__ partial) {
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (c >= n_chunks) return;
    const long long begin = chunks[3 * c + 1], len = chunks[3 * c + 2];
    double s = 0.0;
    if (begin >= 0 && len > 0 && begin + len <= n_order) {
        for (long long e = lane; e < len; e += 64) {
            const long long i = order[begin + e];
            if (i >= 0 && i < n) s += (double)g[i];
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) partial[c] = s;
}

// Second launch: one lane per group.  The group's chunks are consecutive in the table: found by bisection, added in chunk order in f64,
// rounded to f32 once.  A group without chunks gets 0.
__global__ __launch_bounds__(256) void codebook_combine_kernel(const int *__restrict__ chunks, int n_chunks, int n_groups,
                                                               const double *__restrict__ partial, float *__restrict__ gbook) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n_groups) return;
    int lo = 0, hi = n_chunks;                   // the first chunk whose group is >= j
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (chunks[3 * mid] < j) lo = mid + 1; else hi = mid;
    }
    double s = 0.0;
    for (int c = lo; c < n_chunks && chunks[3 * c] == j; ++c) s += partial[c];
    gbook[j] = (float)s;
}

extern "C" int jlm_train_codebook_grad(const float *g, long long n, const int *order, long long n_order, const int *chunks, int n_chunks,
                                       int n_groups, double *partial, float *gbook, void *stream) {
    if (!g || !gbook || n < 1 || n_order < 0 || n_chunks < 0 || n_groups < 1 || (n_chunks > 0 && (!order || !chunks || !partial))) return -1;
    if (n_chunks > 0) {
        hipLaunchKernelGGL(codebook_partial_kernel, dim3((unsigned)((n_chunks + 3) / 4)), dim3(256), 0, (hipStream_t)stream, g, n, order,
                           n_order, chunks, n_chunks, partial);
        JLM_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(codebook_combine_kernel, dim3((unsigned)((n_groups + 255) / 256)), dim3(256), 0, (hipStream_t)stream, chunks,
                       n_chunks, n_groups, partial, gbook);
    JLM_LAUNCH_CHECK();
    return 0;
}
