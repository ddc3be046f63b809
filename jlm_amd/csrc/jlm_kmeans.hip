// jlm_kmeans.hip -- scalar k-means compression of one weight tensor (jlm_kmeans1d, include/jlm_hip.h; jlm_amd/compress.py).  What the
// reference's train/comp.py:20-48 asks of scikit-learn's KMeans: greedy k-means++ seeding, then Lloyd's iteration, n_init = 1.
//
// Every accumulation is an INTEGER sum, so no result depends on the launch shape or on the order atomics land in, and
// jlm_amd/compress.py kmeans_reference restates the arithmetic bit for bit:
//   q = min(rint((x - mn) 2^e), 2^36 - 1) in f64, 2^35 <= (mx - mn) 2^e < 2^36: the Lloyd grid.  Per-centre sums < 2^36 n <= 2^63.
//   v = q >> 18: the seeding grid, 2^18 bins.  D^2 < 2^36, count * D^2 totals <= 2^63.
//
// km_range_kernel   min / max as order-preserving unsigned keys (integer atomicMax), a flag for NaN / infinity.
// km_hist_kernel    counts per seeding bin: LDS integer atomics per (bin range, slice of x), then one flush to the global histogram.
//
// The seeding works on the histogram alone (a draw and a trial's total depend on a value only through its bin), so its cost does not
// depend on n.  The bins are cut into 1024 chunks of 256; S[chunk][t] holds the chunk's count * D^2 as trial t of the last round
// would leave it.  Two launches per round r:
// km_draw_kernel    one workgroup, thread = chunk.  Totals of S per trial (block reduce) -> the last round's winner: the smallest total,
//                   the lowest trial on a tie; its centre is recorded, W = the thread's S for it.  Block scan of W (exclusive prefix,
//                   total) -> the trials' targets floor(u total) -> the drawn bin is the NUMBER of bins whose inclusive prefix is <= the
//                   target (prefixes do not decrease): 256 for every chunk wholly below it (ballot + popcount), and wave t scans the one
//                   chunk that straddles trial t's target, four bins per lane.  r = K: no draw; the K centres are rank-sorted and the
//                   Lloyd start and its midpoint keys written.
// km_eval_kernel    one wave per chunk, four bins per lane: the winner's centre into D (written back), then per trial the chunk's
//                   count * min(D, |v - c_t|)^2, wave-reduced into S.  (r = -1: the plain counts, what centre 0 is drawn from.)
// km_assign_kernel  the Lloyd pass and (FINAL) the code pass: x in 16-byte loads, grid-stride; the K - 1 keys M_j = c_j + c_(j+1) in LDS,
//                   padded to 255 with ~0; code = #{j : M_j < 2 q} by a branch-free 8-step search; per-workgroup count / sum bins in
//                   LDS (integer LDS atomics), one flush per workgroup to the global bins; FINAL: four codes per lane, one 32-bit store.
// km_update_kernel  one workgroup: rounded integer means, largest shift, new keys, bins zeroed, pass counter, the stop flag.  Once the
//                   flag is set the passes already enqueued return at once: the host reads it every JLM_KMEANS_SYNC_EVERY passes.
// km_codebook_kernel  codebook_j = (float)(mn + c_j 2^-e).
#include "jlm_common.h"

#include <math.h>
#include <string.h>

typedef unsigned long long u64;
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

#define KM_SHIFT 18
#define KM_BINS (1 << KM_SHIFT)
#define KM_QMAX ((1ull << 36) - 1ull)
#define KM_CHUNK 256                                    // bins per chunk: one wave, four bins per lane
#define KM_CHUNKS (KM_BINS / KM_CHUNK)                  // 1024: one thread of the draw kernel each
#define KM_DRAW_WAVES (KM_CHUNKS / 64)
#define KM_MAX_TRIALS 8
#define KM_THREADS 256
#define KM_KMAX 256

static_assert(KM_CHUNKS == 1024 && KM_CHUNK == 4 * 64, "a chunk is one wave of 16-byte words; the chunks are one workgroup");

struct KmSeed {                          // the seeding's words
    unsigned c_prev, pad[7];
    unsigned cand[2][KM_MAX_TRIALS];     // [round & 1]: the round's drawn bins
    unsigned seeds[KM_KMAX];             // the chosen bins in round order
};

struct KmState {
    unsigned nmin_key, max_key;          // ~key(min), key(max): both grow under atomicMax from 0
    unsigned nonfinite, done, n_iter, pad[3];
};

// scratch layout (bytes): [0, 256) KmState; then centres, keys, cnt, sum: u64 [256] each; KmSeed; at 16384 the histogram, then the
// distances, then S
#define KM_OFF_CENTRES 256
#define KM_OFF_KEYS (KM_OFF_CENTRES + 2048)
#define KM_OFF_CNT (KM_OFF_KEYS + 2048)
#define KM_OFF_SUM (KM_OFF_CNT + 2048)
#define KM_OFF_SEED (KM_OFF_SUM + 2048)
#define KM_OFF_HIST 16384
#define KM_OFF_DIST (KM_OFF_HIST + 4 * KM_BINS)
#define KM_OFF_S (KM_OFF_DIST + 4 * KM_BINS)
static_assert(KM_OFF_SEED + sizeof(KmSeed) <= KM_OFF_HIST && KM_OFF_S + 8 * KM_MAX_TRIALS * KM_CHUNKS == JLM_KMEANS_SCRATCH_BYTES,
              "scratch layout");

// floats as unsigned keys in the floats' order (-0 below +0)
__host__ __device__ __forceinline__ unsigned km_key(unsigned bits) { return (bits >> 31) ? ~bits : (bits | 0x80000000u); }
__host__ __device__ __forceinline__ unsigned km_unkey(unsigned key) { return (key >> 31) ? (key & 0x7fffffffu) : ~key; }

__device__ __forceinline__ u64 km_quant(float x, double mn, int e) {
    const double s = rint(ldexp((double)x - mn, e));             // >= 0: mn is the minimum of the same values
    const u64 q = s > 0.0 ? (u64)s : 0ull;
    return q < KM_QMAX ? q : KM_QMAX;
}

// sample_rows_kernel's mixer (splitmix64) of (seed, centre, trial): all 64 bits
__device__ __forceinline__ u64 km_mix(u64 seed, unsigned centre, unsigned trial) {
    u64 z = seed + 0x9E3779B97F4A7C15ull * (((u64)centre << 32) | (u64)(trial + 1u));
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__global__ __launch_bounds__(KM_THREADS) void km_range_kernel(const float *__restrict__ x, long long n, KmState *st) {
    const long long n4 = n >> 2;
    const u32x4 *x4 = reinterpret_cast<const u32x4 *>(x);
    unsigned lo = 0xffffffffu, hi = 0u, bad = 0u;
    auto take = [&](unsigned b) {
        bad |= (b & 0x7f800000u) == 0x7f800000u;
        const unsigned k = km_key(b);
        lo = min(lo, k);
        hi = max(hi, k);
    };
    for (long long i = (long long)blockIdx.x * KM_THREADS + threadIdx.x; i < n4; i += (long long)gridDim.x * KM_THREADS) {
        const u32x4 v = x4[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) take(v[j]);
    }
    if (blockIdx.x == 0 && threadIdx.x < (unsigned)(n & 3)) take(reinterpret_cast<const unsigned *>(x)[4 * n4 + threadIdx.x]);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        lo = min(lo, (unsigned)__shfl_xor((int)lo, off));
        hi = max(hi, (unsigned)__shfl_xor((int)hi, off));
        bad |= (unsigned)__shfl_xor((int)bad, off);
    }
    if ((threadIdx.x & 63) == 0) {
        atomicMax(&st->nmin_key, ~lo);
        atomicMax(&st->max_key, hi);
        if (bad) atomicOr(&st->nonfinite, 1u);
    }
}

// Workgroup (p, s) = (blockIdx.x % KM_HIST_RANGES, blockIdx.x / KM_HIST_RANGES) counts the values of slice s that fall into bin range p
// in LDS, then adds its non-empty bins to the global histogram: x is read KM_HIST_RANGES times (cheap) so that the atomics on the
// few thousand bins that hold the bulk of a weight tensor land in LDS, not on a handful of L2 lines.
#define KM_HIST_RANGES 16
#define KM_HIST_RANGE_BINS (KM_BINS / KM_HIST_RANGES)
__global__ __launch_bounds__(KM_THREADS) void km_hist_kernel(const float *__restrict__ x, long long n, double mn, int e, unsigned *hist) {
    __shared__ unsigned s_h[KM_HIST_RANGE_BINS];
    const unsigned p = blockIdx.x % KM_HIST_RANGES, slice = blockIdx.x / KM_HIST_RANGES, slices = gridDim.x / KM_HIST_RANGES;
    const unsigned base = p * KM_HIST_RANGE_BINS;
    for (int i = threadIdx.x; i < KM_HIST_RANGE_BINS; i += KM_THREADS) s_h[i] = 0;
    __syncthreads();
    const long long n4 = n >> 2;
    const f32x4 *x4 = reinterpret_cast<const f32x4 *>(x);
    for (long long i = (long long)slice * KM_THREADS + threadIdx.x; i < n4; i += (long long)slices * KM_THREADS) {
        const f32x4 v = x4[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned b = (unsigned)(km_quant(v[j], mn, e) >> KM_SHIFT) - base;
            if (b < KM_HIST_RANGE_BINS) atomicAdd(&s_h[b], 1u);
        }
    }
    if (slice == 0 && threadIdx.x < (unsigned)(n & 3)) {
        const unsigned b = (unsigned)(km_quant(x[4 * n4 + threadIdx.x], mn, e) >> KM_SHIFT) - base;
        if (b < KM_HIST_RANGE_BINS) atomicAdd(&s_h[b], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < KM_HIST_RANGE_BINS; i += KM_THREADS) {
        const unsigned c = s_h[i];
        if (c) atomicAdd(&hist[base + i], c);
    }
}

__device__ __forceinline__ u64 km_shfl_xor64(u64 v, int off) {
    const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, off), hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), off);
    return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 km_shfl_up64(u64 v, int off) {
    const unsigned lo = (unsigned)__shfl_up((int)(unsigned)v, off), hi = (unsigned)__shfl_up((int)(unsigned)(v >> 32), off);
    return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ unsigned km_absdiff(unsigned a, unsigned b) { return a > b ? a - b : b - a; }

__device__ __forceinline__ u64 km_wave_sum64(u64 s) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += km_shfl_xor64(s, off);
    return s;
}
// inclusive prefix over the wave's lanes
__device__ __forceinline__ u64 km_wave_scan64(u64 inc, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const u64 t = km_shfl_up64(inc, off);
        if (lane >= off) inc += t;
    }
    return inc;
}

// r >= 0: round r's trials (sd->cand[r & 1][0 .. L)) against D after the centre of round r - 1 (sd->c_prev; r = 0: no centre yet, D is
// "infinite").  r < 0: S[chunk][0] = the chunk's count.
__global__ __launch_bounds__(KM_THREADS) void km_eval_kernel(const unsigned *__restrict__ hist, unsigned *dist, const KmSeed *__restrict__ sd,
                                                             u64 *S, int r, int L) {
    const int lane = threadIdx.x & 63, chunk = blockIdx.x * (KM_THREADS / 64) + (threadIdx.x >> 6);
    const int g = chunk * 64 + lane;
    const unsigned v0 = 4u * (unsigned)g;
    const u32x4 h = reinterpret_cast<const u32x4 *>(hist)[g];
    if (r < 0) {
        const u64 s = km_wave_sum64((u64)h[0] + h[1] + h[2] + h[3]);
        if (lane == 0) S[chunk * KM_MAX_TRIALS] = s;
        return;
    }
    u32x4 d = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
    if (r > 0) {
        const unsigned c_prev = sd->c_prev;
        d = reinterpret_cast<const u32x4 *>(dist)[g];
#pragma unroll
        for (int i = 0; i < 4; ++i) d[i] = min(d[i], km_absdiff(v0 + i, c_prev));
    }
    reinterpret_cast<u32x4 *>(dist)[g] = d;
#pragma unroll
    for (int t = 0; t < KM_MAX_TRIALS; ++t)
        if (t < L) {
            const unsigned c = sd->cand[r & 1][t];
            u64 s = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const unsigned m = min(d[i], km_absdiff(v0 + i, c));
                s += (u64)h[i] * ((u64)m * m);
            }
            s = km_wave_sum64(s);
            if (lane == 0) S[chunk * KM_MAX_TRIALS + t] = s;
        }
}

// round r < K: the winner of round r - 1 among its Lprev trials (r = 0: S holds the counts, Lprev = 1), then this round's L draws.
// r = K: the winner of the last round, then the sorted Lloyd start.
__global__ __launch_bounds__(KM_CHUNKS) void km_draw_kernel(const unsigned *__restrict__ hist, const unsigned *__restrict__ dist, KmSeed *sd,
                                                            const u64 *__restrict__ S, u64 *centres, u64 *keys, int r, int K, int Lprev, int L,
                                                            u64 seed) {
    __shared__ u64 s_part[KM_DRAW_WAVES][KM_MAX_TRIALS];
    __shared__ u64 s_wave[KM_DRAW_WAVES];
    __shared__ unsigned s_idx[KM_MAX_TRIALS], s_chunk[KM_MAX_TRIALS];
    __shared__ u64 s_rem[KM_MAX_TRIALS];
    __shared__ unsigned s_c[KM_KMAX];
    __shared__ u64 s_sorted[KM_KMAX];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;

    u64 mine[KM_MAX_TRIALS];
#pragma unroll
    for (int t = 0; t < KM_MAX_TRIALS; ++t) {
        mine[t] = t < Lprev ? S[tid * KM_MAX_TRIALS + t] : 0;
        if (t < Lprev) {
            const u64 s = km_wave_sum64(mine[t]);
            if (lane == 0) s_part[wv][t] = s;
        }
    }
    if (tid < KM_MAX_TRIALS) s_idx[tid] = 0;
    __syncthreads();
    int win = 0;
    u64 total = ~0ull;
#pragma unroll
    for (int t = 0; t < KM_MAX_TRIALS; ++t)
        if (t < Lprev) {
            u64 s = 0;
#pragma unroll
            for (int w = 0; w < KM_DRAW_WAVES; ++w) s += s_part[w][t];
            if (s < total) { total = s; win = t; }
        }
    u64 W = 0;
#pragma unroll
    for (int t = 0; t < KM_MAX_TRIALS; ++t)
        if (t == win) W = mine[t];
    const unsigned c_prev = r > 0 ? sd->cand[(r - 1) & 1][win] : 0u;
    if (tid == 0 && r > 0) {
        sd->seeds[r - 1] = c_prev;
        sd->c_prev = c_prev;
    }
    if (r == K) {
        // rank sort (equal centres keep their round order), then the Lloyd start and its midpoint keys
        if (tid < K) s_c[tid] = tid == K - 1 ? c_prev : sd->seeds[tid];
        __syncthreads();
        if (tid < K) {
            const unsigned c = s_c[tid];
            int rank = 0;
            for (int i = 0; i < K; ++i) rank += s_c[i] < c || (s_c[i] == c && i < tid);
            s_sorted[rank] = ((u64)c << KM_SHIFT) + (1ull << (KM_SHIFT - 1));
        }
        __syncthreads();
        if (tid < KM_KMAX) {
            if (tid < K) centres[tid] = s_sorted[tid];
            keys[tid] = tid < K - 1 ? s_sorted[tid] + s_sorted[tid + 1] : ~0ull;
        }
        return;
    }
    if (total == 0) {                                    // every value sits on a centre: repeat the last one
        if (tid < L) sd->cand[r & 1][tid] = c_prev;
        return;
    }
    const u64 inc = km_wave_scan64(W, lane);
    if (lane == 63) s_wave[wv] = inc;
    __syncthreads();
    u64 excl = inc - W;
#pragma unroll
    for (int w = 0; w < KM_DRAW_WAVES; ++w)
        if (w < wv) excl += s_wave[w];
#pragma unroll
    for (int t = 0; t < KM_MAX_TRIALS; ++t)
        if (t < L) {
            const u64 tg = __umul64hi(km_mix(seed, (unsigned)r, (unsigned)t), total);
            const unsigned long long below = __ballot(excl + W <= tg);
            if (lane == 0 && below) atomicAdd(&s_idx[t], (unsigned)KM_CHUNK * (unsigned)__popcll(below));
            if (excl <= tg && tg < excl + W) { s_chunk[t] = (unsigned)tid; s_rem[t] = tg - excl; }      // exactly one chunk
        }
    __syncthreads();
    if (wv < L) {                                        // wave t: the chunk that straddles trial t's target
        const int chunk = (int)s_chunk[wv];
        const u64 rem = s_rem[wv];
        const int g = chunk * 64 + lane;
        const unsigned v0 = 4u * (unsigned)g;
        const u32x4 h = reinterpret_cast<const u32x4 *>(hist)[g];
        u64 w[4];
        if (r > 0) {
            const u32x4 d = reinterpret_cast<const u32x4 *>(dist)[g];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const unsigned m = min(d[i], km_absdiff(v0 + i, c_prev));
                w[i] = (u64)h[i] * ((u64)m * m);
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) w[i] = h[i];
        }
        const u64 ls = w[0] + w[1] + w[2] + w[3];
        u64 run = km_wave_scan64(ls, lane) - ls;
        unsigned cnt = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            run += w[i];
            cnt += run <= rem;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) cnt += (unsigned)__shfl_xor((int)cnt, off);
        if (lane == 0) sd->cand[r & 1][wv] = s_idx[wv] + cnt;
    }
}

// code = #{j < 255 : keys[j] < 2 q}: keys ascending, padded with ~0
__device__ __forceinline__ unsigned km_search(const u64 *sk, u64 q2) {
    unsigned pos = 0;
#pragma unroll
    for (unsigned s = 128; s >= 1; s >>= 1) pos += sk[pos + s - 1] < q2 ? s : 0u;
    return pos;
}

template <int FINAL>
__global__ __launch_bounds__(KM_THREADS) void km_assign_kernel(const float *__restrict__ x, long long n, double mn, int e, const KmState *st,
                                                               const u64 *__restrict__ keys, u64 *cnt, u64 *sum, unsigned char *code) {
    if (!FINAL && st->done) return;
    __shared__ u64 sk[KM_KMAX];
    __shared__ u64 s_sum[KM_KMAX];
    __shared__ unsigned s_cnt[KM_KMAX];
    const int tid = threadIdx.x;
    sk[tid] = tid < KM_KMAX - 1 ? keys[tid] : ~0ull;
    s_sum[tid] = 0;
    s_cnt[tid] = 0;
    __syncthreads();
    const long long n4 = n >> 2;
    const f32x4 *x4 = reinterpret_cast<const f32x4 *>(x);
    for (long long i = (long long)blockIdx.x * KM_THREADS + tid; i < n4; i += (long long)gridDim.x * KM_THREADS) {
        const f32x4 v = x4[i];
        unsigned packed = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const u64 q = km_quant(v[j], mn, e);
            const unsigned c = km_search(sk, 2 * q);
            if (FINAL) packed |= c << (8 * j);
            else { atomicAdd(&s_cnt[c], 1u); atomicAdd(&s_sum[c], q); }
        }
        if (FINAL) reinterpret_cast<unsigned *>(code)[i] = packed;
    }
    if (blockIdx.x == 0 && tid < (int)(n & 3)) {
        const u64 q = km_quant(x[4 * n4 + tid], mn, e);
        const unsigned c = km_search(sk, 2 * q);
        if (FINAL) code[4 * n4 + tid] = (unsigned char)c;
        else { atomicAdd(&s_cnt[c], 1u); atomicAdd(&s_sum[c], q); }
    }
    if (!FINAL) {
        __syncthreads();
        if (s_cnt[tid]) { atomicAdd(&cnt[tid], (u64)s_cnt[tid]); atomicAdd(&sum[tid], s_sum[tid]); }
    }
}

__global__ __launch_bounds__(KM_KMAX) void km_update_kernel(KmState *st, u64 *centres, u64 *keys, u64 *cnt, u64 *sum, int K, u64 thr) {
    __shared__ u64 s_c[KM_KMAX];
    __shared__ u64 s_shift;
    const int tid = threadIdx.x;
    const unsigned done = st->done;
    if (tid == 0) s_shift = 0;
    __syncthreads();
    if (done) return;
    if (tid < K) {
        const u64 c = centres[tid], m = cnt[tid];
        const u64 nc = m ? (sum[tid] + m / 2) / m : c;
        centres[tid] = nc;
        s_c[tid] = nc;
        atomicMax(&s_shift, nc > c ? nc - c : c - nc);
    }
    cnt[tid] = 0;
    sum[tid] = 0;
    __syncthreads();
    keys[tid] = tid < K - 1 ? s_c[tid] + s_c[tid + 1] : ~0ull;
    if (tid == 0) {
        st->n_iter += 1;
        if (s_shift <= thr) st->done = 1;
    }
}

__global__ __launch_bounds__(KM_KMAX) void km_codebook_kernel(const u64 *centres, int K, double mn, int e, float *codebook) {
    const int tid = threadIdx.x;
    if (tid < K) codebook[tid] = (float)(mn + ldexp((double)centres[tid], -e));
}

static const int km_trials[9] = {0, 2, 3, 4, 4, 5, 6, 6, 7};            // 2 + floor(ln 2^bit)

#define KM_HIP(call)                          \
    do {                                      \
        hipError_t e__ = (call);              \
        if (e__ != hipSuccess) { rc = (int)e__; goto out; } \
    } while (0)

extern "C" int jlm_kmeans1d(const float *x, long long n, int bit, uint64_t seed, int max_iter, double tol, unsigned char *code, float *codebook,
                            void *scratch, int grid, int *info_host, float *ms_host, void *stream) {
    if (!x || !code || !codebook || !scratch || !info_host || n < 1 || n > JLM_KMEANS_MAX_N || bit < 1 || bit > 8 || max_iter < 1 ||
        !(tol >= 0.0) || !(tol < INFINITY) || grid < 0 || ((uintptr_t)x & 15) || ((uintptr_t)code & 3) || ((uintptr_t)scratch & 15))
        return -1;
    hipStream_t st = (hipStream_t)stream;
    const int K = 1 << bit;
    char *sc = (char *)scratch;
    KmState *state = (KmState *)sc;
    u64 *centres = (u64 *)(sc + KM_OFF_CENTRES), *keys = (u64 *)(sc + KM_OFF_KEYS), *cnt = (u64 *)(sc + KM_OFF_CNT), *sum = (u64 *)(sc + KM_OFF_SUM);
    unsigned *hist = (unsigned *)(sc + KM_OFF_HIST), *dist = (unsigned *)(sc + KM_OFF_DIST);
    KmSeed *sd = (KmSeed *)(sc + KM_OFF_SEED);
    u64 *S = (u64 *)(sc + KM_OFF_S);
    int rc = 0;
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    KmState hs;
    info_host[0] = info_host[1] = info_host[2] = info_host[3] = 0;
    if (ms_host) for (int i = 0; i < 5; ++i) ms_host[i] = 0.0f;
    {
        if (grid == 0) {
            int dev = 0, cus = 0;
            KM_HIP(hipGetDevice(&dev));
            KM_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
            grid = 4 * (cus > 0 ? cus : 1);
        }
        const long long need = ((n >> 2) + KM_THREADS - 1) / KM_THREADS;
        if (grid > need) grid = need > 0 ? (int)need : 1;
        if (ms_host) for (int i = 0; i < 6; ++i) KM_HIP(hipEventCreate(&ev[i]));
#define KM_MARK(i) do { if (ms_host) KM_HIP(hipEventRecord(ev[i], st)); } while (0)
        KM_HIP(hipMemsetAsync(sc, 0, KM_OFF_DIST, st));
        KM_MARK(0);
        km_range_kernel<<<grid, KM_THREADS, 0, st>>>(x, n, state);
        KM_HIP(hipGetLastError());
        KM_MARK(1);
        KM_HIP(hipMemcpyAsync(&hs, state, sizeof(hs), hipMemcpyDeviceToHost, st));
        KM_HIP(hipStreamSynchronize(st));
        if (hs.nonfinite) { info_host[2] = 1; goto out; }
        unsigned lo_bits = km_unkey(~hs.nmin_key), hi_bits = km_unkey(hs.max_key);
        float mn_f, mx_f;
        memcpy(&mn_f, &lo_bits, 4);
        memcpy(&mx_f, &hi_bits, 4);
        const double mn = (double)mn_f, rng = (double)mx_f - (double)mn_f;
        if (!(rng > 0.0)) {                              // constant: codebook all mn (+0 for -0), codes 0
            float book[KM_KMAX];
            for (int j = 0; j < K; ++j) book[j] = mn_f + 0.0f;
            KM_HIP(hipMemsetAsync(code, 0, (size_t)n, st));
            KM_HIP(hipMemcpyAsync(codebook, book, sizeof(float) * K, hipMemcpyHostToDevice, st));
            KM_HIP(hipStreamSynchronize(st));
            info_host[1] = 1;
            goto out;
        }
        int ex = 0;
        (void)frexp(rng, &ex);
        const int e = 36 - ex;                           // 2^35 <= rng 2^e < 2^36
        const double thr_d = floor(tol * ldexp(rng, e));
        const u64 thr = thr_d >= 9223372036854775808.0 ? (1ull << 63) : (u64)thr_d;
        {
            const long long need = ((n >> 2) + KM_THREADS - 1) / KM_THREADS;
            const int slices = need >= 16 ? 16 : (need > 0 ? (int)need : 1);
            km_hist_kernel<<<KM_HIST_RANGES * slices, KM_THREADS, 0, st>>>(x, n, mn, e, hist);
        }
        KM_HIP(hipGetLastError());
        KM_MARK(2);
        {
            const int trials = km_trials[bit], eval_grid = KM_CHUNKS / (KM_THREADS / 64);
            km_eval_kernel<<<eval_grid, KM_THREADS, 0, st>>>(hist, dist, sd, S, -1, 1);
            for (int r = 0; r <= K; ++r) {
                const int L = r ? trials : 1;
                km_draw_kernel<<<1, KM_CHUNKS, 0, st>>>(hist, dist, sd, S, centres, keys, r, K, r <= 1 ? 1 : trials, L, (u64)seed);
                if (r < K) km_eval_kernel<<<eval_grid, KM_THREADS, 0, st>>>(hist, dist, sd, S, r, L);
            }
        }
        KM_HIP(hipGetLastError());
        KM_MARK(3);
        for (int it = 0; it < max_iter;) {
            const int stop = it + JLM_KMEANS_SYNC_EVERY < max_iter ? it + JLM_KMEANS_SYNC_EVERY : max_iter;
            for (; it < stop; ++it) {
                km_assign_kernel<0><<<grid, KM_THREADS, 0, st>>>(x, n, mn, e, state, keys, cnt, sum, nullptr);
                km_update_kernel<<<1, KM_KMAX, 0, st>>>(state, centres, keys, cnt, sum, K, thr);
            }
            KM_HIP(hipGetLastError());
            KM_HIP(hipMemcpyAsync(&hs, state, sizeof(hs), hipMemcpyDeviceToHost, st));
            KM_HIP(hipStreamSynchronize(st));
            if (hs.done) break;
        }
        info_host[0] = (int)hs.n_iter;
        KM_MARK(4);
        km_assign_kernel<1><<<grid, KM_THREADS, 0, st>>>(x, n, mn, e, state, keys, cnt, sum, code);
        km_codebook_kernel<<<1, KM_KMAX, 0, st>>>(centres, K, mn, e, codebook);
        KM_HIP(hipGetLastError());
        KM_MARK(5);
        KM_HIP(hipStreamSynchronize(st));
        if (ms_host)
            for (int i = 0; i < 5; ++i) KM_HIP(hipEventElapsedTime(&ms_host[i], ev[i], ev[i + 1]));
    }
out:
    for (int i = 0; i < 6; ++i)
        if (ev[i]) (void)hipEventDestroy(ev[i]);
    return rc;
}
