// jlm_frame_tail.hip -- the tail of a decode frame between the T projection and the normaliser as ONE launch (jlm_pack_edge_mx6,
// include/jlm_hip.h): the mx6 packing of the frame's live T rows (pack_t_mx6_kernel, jlm_mixed.hip) and the edge logits of the words that
// start in the frame's cells (wordlist_kernel<0>, jlm_beam.hip).
//
// The edge-logit workgroup of a (frame, sentence) cell stages exactly that cell's rows of T in LDS, and the live cells' rows ARE the frame's
// live rows -- the packer's whole input: row g0[cell] + slot sits at compact position live_base[cell] + slot (beam_step_kernel).  So the
// workgroup packs its rows from LDS: one launch and one pass over T less per frame.  Both halves keep their arithmetic to the bit: the
// quantiser is the stand-alone packer's (jlm_mx6_pack.h), the dot products are wordlist_kernel<0>'s -- eight lanes per word, fmaf over
// kc = sub, sub + 8, ... in element order, xor-shuffle adds 1, 2, 4, + b2[w].
//
// What differs is the order of the memory round trips, which is all the edge-logit kernel's time (one workgroup per CU, one wave per
// SIMD: nothing hides a wait): every index (cell count, rows, word-list bounds) and the word ids of the first TWO passes are requested
// before anything is waited for, and the rows go to LDS by LDS-DMA (no staging registers) while the first pass's weight rows and biases
// are gathered.  The dot products take the cell's rows in groups of FT_RG = 4 while the word's weight-row granules bv[8] are held (each
// accumulator's chain is its own: same bits), rows and cells are scalar: 64 registers, no scratch, at most 32 KB of LDS -- the budget
// of a guest beside a resident normaliser workgroup.
//
// Two departures from the plan this kernel was written to (both keep the bits):
//   - the pack runs LAST, behind the edge logits, not under the weight-row gathers: a word's bv[] (32 registers) and the quantiser (43)
//     do not fit 64 registers together.  What is saved is the packer's launch and its pass over T in memory, not its VALU time.
//   - the sum over a word's eight lanes is three DPP moves (quad_perm, quad_perm, row_half_mirror), not three __shfl_xor: ft_sum8 says
//     why lane 0 ends with the same bits.
#include "jlm_common.h"
#include "jlm_mx6_pack.h"
using namespace jlm_mx;

#define FT_THREADS 256
#define FT_ROWS 16        // rows of a cell: beam <= 16 (jlm_beam.hip WL_ROWS)
#define FT_RG 4           // rows per group of the dot products

#define GLDS16(gp, lp)                                                                          \
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(gp),      \
                                     (__attribute__((address_space(3))) void *)(lp), 16, 0, 0)

// every wave waits for its own LDS-DMA before the barrier: behind it the cell's rows are in LDS (the wait also covers the gathers issued
// before it, which the code behind the barrier needs at once)
#define FT_SYNC_DMA()                                   \
    do {                                                \
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); \
        __syncthreads();                                \
    } while (0)

namespace {

typedef __attribute__((address_space(3))) float lds_f32;
typedef __attribute__((address_space(3))) f32x4 lds_f32x4;

// Sum over the 8 lanes of a word, in lane sub = 0 the bits of wordlist_kernel's three xor-shuffle adds (1, 2, 4): after the steps 1 and 2
// the four lanes of a quad hold the SAME bits (IEEE addition commutes), so the partner of step 4 may be any lane of the other quad --
// row_half_mirror's 7 - sub instead of sub ^ 4 -- and the three steps are DPP moves instead of LDS-crossbar round trips.
__device__ __forceinline__ float ft_sum8(float v) {
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xf, 0xf, false));       // quad_perm(1,0,3,2)
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xf, 0xf, false));       // quad_perm(2,3,0,1)
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xf, 0xf, false));      // row_half_mirror
    return v;
}

// a word's weight-row granules, bias and place in T: what a pass waits for
struct FtWord {
    f32x4 bv[8];
    float bias;
    int K4, toff, out;        // out: the word's row of edge[]
};

// Lanes without a word, and granules past the word's row (kc >= K4), read a granule that exists instead of branching round the load:
// the dot products skip them (K4 = 0 for a lane without a word), so what they hold is never used.
__device__ __forceinline__ void ft_gather(const SegTable &segs, const float *__restrict__ b2, const int *__restrict__ wl_out, int at, int w, bool valid,
                                          int sub, FtWord &g) {
    int K4 = 0, toff = 0;
    const float *brow_f = segs.s[0].B;
    for (int si = 0; si < segs.n; ++si)
        if (valid && w >= segs.s[si].v_start && w < segs.s[si].v_end) {
            K4 = segs.s[si].k >> 2;
            toff = segs.s[si].t_off;
            brow_f = segs.s[si].B + (size_t)(w - segs.s[si].v_start) * segs.s[si].ldb;
        }
    const f32x4 *brow = reinterpret_cast<const f32x4 *>(brow_f);
    // the word's whole share of the weight row in one round trip (k <= 256: at most 8 x 16 B per lane)
#pragma unroll
    for (int c8 = 0; c8 < 8; ++c8) g.bv[c8] = brow[max(min(sub + 8 * c8, K4 - 1), 0)];
    g.bias = b2[valid ? w : 0];
    g.out = wl_out[valid ? at : 0];
    g.K4 = K4;
    g.toff = toff;
}

// One workgroup per cell j of the frame (sentence j: the per-frame arrays g0v, cnt_idx, wl_idx, live_base are the frame's slices).
__global__ __launch_bounds__(FT_THREADS, 8) void frame_tail_mx6_kernel(
    SegTable segs, MxTArgs pa, const float *__restrict__ b2, const float *__restrict__ T, int ldt, const int *__restrict__ g0v,
    const int *__restrict__ cnt, const int *__restrict__ cnt_idx, const int *__restrict__ wl, const int *__restrict__ wl_off,
    const int *__restrict__ wl_idx, int wl_base, const int *__restrict__ wl_out, float *__restrict__ edge, int beam,
    const int *__restrict__ sent_len, const int *__restrict__ live_base, int frame, unsigned char *__restrict__ Tm, int ld_tm) {
    extern __shared__ __attribute__((aligned(16))) float sm[];      // [FT_ROWS][ldt], rounded up to whole LDS-DMA instructions (1 KB)
    const int j = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // ---- 1. everything that does not depend on T, requested up front.  The cell's indices take TWO round trips, not one per index: five
    // lanes load the five first-level words in one instruction (every wave for itself), three lanes the three they point to.
    const int *p1 = lane == 0 ? cnt_idx + j : lane == 1 ? g0v + j : lane == 2 ? live_base + j : lane == 3 ? sent_len + j : wl_idx + j;
    const int v1 = *p1;
    const int ci = __builtin_amdgcn_readlane(v1, 0), gbase = __builtin_amdgcn_readlane(v1, 1), lbase = __builtin_amdgcn_readlane(v1, 2);
    const int slen = __builtin_amdgcn_readlane(v1, 3), lid = wl_base + __builtin_amdgcn_readlane(v1, 4);
    const int *p2 = lane == 0 ? cnt + ci : wl_off + lid + (lane == 1 ? 0 : 1);
    const int v2 = *p2;
    const int c = __builtin_amdgcn_readlane(v2, 0), w0 = __builtin_amdgcn_readlane(v2, 1), nw = __builtin_amdgcn_readlane(v2, 2) - w0;
    const int nrows = min(c, beam);
    if (nrows <= 0) return;
    // live: the cell's rows are in the frame's live list (a sentence's FINAL cell has rows too, but they are not listed and its
    // live_base is stale: it is not packed)
    const bool live = frame < slen;
    if (!live && nw == 0) return;
    const int sub = tid & 7, slot = tid >> 3;
    int w_cur = -1, w_nxt = -1;
    if (slot < nw) w_cur = wl[w0 + slot];
    if (FT_THREADS / 8 + slot < nw) w_nxt = wl[w0 + FT_THREADS / 8 + slot];
    {   // the cell's rows T[gbase .. gbase + nrows) (consecutive in g) -> LDS, 1 KB per instruction and wave; the lanes past the end of the
        // last instruction re-read the last granule into the slack behind the rows
        const int total16 = nrows * (ldt >> 2);
        const int n_inst = (total16 + 63) >> 6;
        const char *src = reinterpret_cast<const char *>(T + (size_t)gbase * ldt);
        for (int i = wave; i < n_inst; i += FT_THREADS / 64) GLDS16(src + 16 * (size_t)min(i * 64 + lane, total16 - 1), sm + i * 256);
    }
    // ---- 3. edge logits, FT_RG rows at a time out of LDS while the word's bv[] is held: an accumulator's chain (c8 ascending, elements in
    // order) does not depend on how the rows are grouped.  Rows past nrows of the last group read LDS that holds no row (inside the
    // allocation) and are not stored.
    if (nw <= 0) FT_SYNC_DMA();
    for (int wb = 0; wb < nw; wb += FT_THREADS / 8) {
        FtWord g;
        // (the word ids of the first two passes were requested with the indices; a cell with more than 64 words asks for the rest here)
        if (wb >= 2 * (FT_THREADS / 8) && wb + slot < nw) w_cur = wl[w0 + wb + slot];
        ft_gather(segs, b2, wl_out, w0 + wb + slot, w_cur, wb + slot < nw, sub, g);
        w_cur = w_nxt;
        if (wb == 0) FT_SYNC_DMA();
        // (32-bit LDS addresses: a row's granule c8 is an immediate offset of the read)
        const lds_f32 *trow = (const lds_f32 *)sm + g.toff + 4 * sub;
        const int n8 = (g.K4 - sub + 7) >> 3;          // this lane's granules: kc = sub + 8 c8 < K4 (<= 64: the launcher refuses k > 256)
        for (int r0 = 0; r0 < nrows; r0 += FT_RG) {
            float acc[FT_RG];
#pragma unroll
            for (int r = 0; r < FT_RG; ++r) acc[r] = 0.0f;
#pragma unroll
            for (int c8 = 0; c8 < 8; ++c8) {
                if (c8 >= n8) continue;
                // the group's four LDS reads are pinned together in front of the arithmetic: left alone, hipcc (at its register limit) issues
                // one, waits, multiplies, issues the next -- four LDS latencies per granule instead of one
                f32x4 tv[FT_RG];
#pragma unroll
                for (int r = 0; r < FT_RG; ++r) tv[r] = *reinterpret_cast<const lds_f32x4 *>(trow + (r0 + r) * ldt + 32 * c8);
                asm volatile("" : "+v"(tv[0]), "+v"(tv[1]), "+v"(tv[2]), "+v"(tv[3]));
#pragma unroll
                for (int r = 0; r < FT_RG; ++r) {
                    acc[r] = fmaf(g.bv[c8][0], tv[r][0], acc[r]);
                    acc[r] = fmaf(g.bv[c8][1], tv[r][1], acc[r]);
                    acc[r] = fmaf(g.bv[c8][2], tv[r][2], acc[r]);
                    acc[r] = fmaf(g.bv[c8][3], tv[r][3], acc[r]);
                }
            }
#pragma unroll
            for (int r = 0; r < FT_RG; ++r) acc[r] = ft_sum8(acc[r]);
            if (sub == 0 && wb + slot < nw) {
#pragma unroll
                for (int r = 0; r < FT_RG; ++r)
                    if (r0 + r < nrows) edge[(size_t)g.out * beam + (r0 + r)] = acc[r] + g.bias;
            }
        }
    }
    // ---- 2. pack: the waves share the rows of a live cell, four apart, from LDS into Tm at compact row live_base + slot.  It comes LAST: a
    // word's bv[] (32 registers) and the quantiser (43) do not fit 64 registers together, so the quantiser cannot run under the gathers
    if (!live) return;
    int groups = 0;
    for (int si = 0; si < pa.n_segs; ++si) groups += 2 * pa.seg[si].nb;
    const int n_chunks = (groups + 31) >> 5;
    // (rows 3 - wave, 7 - wave, ...: the words of a short last pass sit in the LOWEST waves, which therefore arrive here last -- they get
    //  the fewest rows)
    for (int r = FT_THREADS / 64 - 1 - wave; r < nrows; r += FT_THREADS / 64)
        for (int ch = 0; ch < n_chunks; ++ch) mx6_pack_t_row(pa, sm + (size_t)r * ldt, lbase + r, ch, lane, Tm, ld_tm);
}

size_t ft_lds_bytes(int ldt) { return ((size_t)FT_ROWS * ldt * sizeof(float) + 1023) / 1024 * 1024; }

}  // namespace

// LDS of a launch at row stride ldt (floats): the residency test asks
extern "C" int jlm_pack_edge_mx6_lds_bytes(int ldt) { return ldt > 0 && ldt % 4 == 0 ? (int)ft_lds_bytes(ldt) : -1; }

extern "C" int jlm_pack_edge_mx6(const jlm_segment *segs_host, int n_segs, const float *b2, const jlm_segment *mixed_segs, const float *t_scale,
                                 int n_mixed, const float *T, int ldt, const int *g0, const int *cnt, const int *cnt_idx, const int *wl,
                                 const int *wl_off, const int *wl_idx, int wl_base, const int *wl_out, float *edge, int beam, int n_groups,
                                 const int *sent_len, const int *live_base, int frame, void *Tm, int ld_tm, void *stream) {
    if (n_segs < 1 || n_segs > JLM_MAX_SEGMENTS || n_mixed < 1 || n_mixed > JLM_MAX_SEGMENTS || ldt <= 0 || ldt % 4 || beam < 1 || !sent_len ||
        !live_base || !Tm)
        return -1;
    if (beam > FT_ROWS) return -2;
    SegTable t;
    t.n = n_segs;
    for (int i = 0; i < n_segs; ++i) {
        t.s[i] = segs_host[i];
        if (t.s[i].k % 4 || t.s[i].ldb % 4 || t.s[i].t_off % 4) return -1;
        if (t.s[i].k > 256) return -2;                       // (a lane holds a word's whole share of the weight row: 8 x 16 B)
    }
    {
        const int want = jlm_mixed_t_stride(mixed_segs, n_mixed);
        if (want == -2) return -2;
        if (ld_tm != want) return -1;
    }
    MxTArgs a;
    int row_bytes = 0;
    if (mx_t_args(mixed_segs, t_scale, n_mixed, 8, a, &row_bytes)) return -2;
    const size_t lds = ft_lds_bytes(ldt);
    if (lds > 32 * 1024) return -2;
    if (n_groups <= 0) return 0;
    hipLaunchKernelGGL(frame_tail_mx6_kernel, dim3(n_groups), dim3(FT_THREADS), lds, (hipStream_t)stream, t, a, b2, T, ldt, g0, cnt, cnt_idx, wl,
                       wl_off, wl_idx, wl_base, wl_out, edge, beam, sent_len, live_base, frame, reinterpret_cast<unsigned char *>(Tm), ld_tm);
    JLM_LAUNCH_CHECK();
    return 0;
}
