// jlm_mx6_pack.h -- packing of hypothesis rows (T, f32) into mx6 rows (jlm_mx6_body.h): the segment table of the row packers and the ONE
// definition of the quantiser's arithmetic, shared by the stand-alone packer (pack_t_mx6_kernel, jlm_mixed.hip: rows from memory) and the
// fused frame tail (frame_tail_mx6_kernel, jlm_frame_tail.hip: a cell's rows from LDS).
#pragma once
#include "jlm_mx6_body.h"

namespace jlm_mx {

struct MxTSeg { int k, t_off, nb, tm_off; float t_scale, tc; };      // tc = 0: no bias columns (k = 32 nb)
struct MxTArgs { int n_segs; MxTSeg seg[JLM_MAX_SEGMENTS]; };

// blocks per row of a segment as its ldb says: ceil((k + 2) / 32) (bias columns) or, for k a multiple of 32, k / 32 (none); -1: neither
static inline int mx_seg_blocks(const jlm_segment &sg) {
    if (sg.k <= 0 || sg.ldb % 32) return -1;
    const int nb = sg.ldb / 32;
    return (nb == (sg.k + 2 + 31) / 32 || nb == (sg.k + 31) / 32) ? nb : -1;
}

// The packers' segment table from the host's segments (t_scale[i] = 2^eT_i); *row_bytes: the bytes of a row's blocks (64 per 16-value
// group).  -2: a shape the packers do not take (max_nb: MXW_MAX_NB for int8 rows, 8 for mx6 rows -- a row's scale bytes, eight per half).
static inline int mx_t_args(const jlm_segment *segs_host, const float *t_scale, int n_segs, int max_nb, MxTArgs &a, int *row_bytes) {
    a.n_segs = n_segs;
    int off = 0;
    for (int i = 0; i < n_segs; ++i) {
        const jlm_segment &sg = segs_host[i];
        const int nb = mx_seg_blocks(sg);
        if (nb < 1 || nb > max_nb || sg.k % 4 || sg.t_off % 4) return -2;
        a.seg[i] = MxTSeg{sg.k, sg.t_off, nb, off, t_scale[i] * 1.4426950408889634f, sg.k + 2 <= 32 * nb ? t_scale[i] : 0.0f};
        off += nb * 128;
    }
    *row_bytes = off;
    return 0;
}

// One wave packs the 16-value groups 32 chunk .. 32 chunk + 31 of ONE row: trow = the row's f32 values (memory or LDS), r = its COMPACT
// position in Tm (granule-major blocks of 32 rows, jlm_mixed_body.h).  A lane owns ONE PLANE of one group of the row's segments (lanes
// 0-31: the lo6 plane of the chunk's groups, lanes 32-63: the hi6 plane of the same groups) -- the quantiser is ~20 VALU instructions per
// value, and with a lane per group and BOTH planes (the int8 packer's assignment) the launch took 12-14 us where the int8 one takes 9.
// The halves are SWAPPED against the vocabulary rows (half 0 = lo6, half 1 = hi6): the instruction pairs k-slot with k-slot.
// r, trow and chunk are wave-uniform (the callers hold them in scalar registers).
__device__ __forceinline__ void mx6_pack_t_row(const MxTArgs &a, const float *trow, int r, int chunk, int lane, unsigned char *__restrict__ Tm,
                                               int ld_tm) {
    const int sl = lane >> 5;                         // plane: 0 = lo6 (half 0 of the row format), 1 = hi6
    unsigned char *oblk = Tm + mx_tm_block(r, ld_tm);
    int total = 0;
    for (int si = 0; si < a.n_segs; ++si) total += 2 * a.seg[si].nb;
    const int g0 = chunk * 32;
    const int grp = g0 + (lane & 31);
    int si = 0, base = 0;
    while (si + 1 < a.n_segs && grp >= base + 2 * a.seg[si].nb) { base += 2 * a.seg[si].nb; ++si; }
    const bool act = grp < total;
    const MxTSeg sg = a.seg[si];
    const int gs = grp - base;                    // group inside the segment: block gs >> 1, half gs & 1 (partner lane ^ 1: base is even)
    f32x4 v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int k0 = 16 * gs + 4 * q;
        v[q] = *reinterpret_cast<const f32x4 *>(reinterpret_cast<const char *>(trow) + 4u * (unsigned)(sg.t_off + ((act && k0 < sg.k) ? k0 : 0)));
    }
    // (k is a multiple of 4 -- mx_t_args refuses any other (`sg.k % 4`), and this placement breaks if it ever stops doing so:
    //  the bias constants can only sit at e = 0, 4, 8, 12 and the slot behind)
    const int d = act ? sg.k - 16 * gs : -2;      // values e < d of the group are real, e = d and d + 1 the bias constants
    const float tc1 = sg.tc * (1.0f / 2048.0f);
    const int j = gs >> 1, half = gs & 1;
    unsigned h_even = 0;
    unsigned hw[4];                               // this lane's eight f16 (values 8 sl .. 8 sl + 7), two to a dword
    float val[16];
    float amax = 0.0f;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const bool real = e < d;
        const float c = (e & 3) == 0 ? (e == d ? sg.tc : 0.0f) : (e & 3) == 1 ? (e == d + 1 ? tc1 : 0.0f) : 0.0f;
        float x = real ? v[e >> 2][e & 3] * sg.t_scale : c;
        asm volatile("" : "+v"(x));               // (the scaled value is used twice: jlm_common.h jlm_split2)
        _Float16 h = (_Float16)x;
        asm volatile("" : "+v"(h));
        val[e] = real ? (sl ? (float)h : x - (float)h) : 0.0f;
        amax = fmaxf(amax, fabsf(val[e]));
        // the f16 part is kept two to a dword and only the half this lane stores: eight registers less than the sixteen f16 held singly
        const unsigned hb = __builtin_bit_cast(unsigned short, h);
        if (e & 1) {
            const unsigned pair = h_even | (hb << 16);
            hw[(e & 7) >> 1] = (e < 8 || sl) ? pair : hw[(e & 7) >> 1];
        } else {
            h_even = hb;
        }
    }
    amax = fmaxf(amax, __shfl_xor(amax, 1));
    if (act) {
        // the f16 part: granules 2 half, 2 half + 1 of the block -- one each from the group's two lanes
        *reinterpret_cast<i32x4 *>(oblk + (unsigned)mx_tm_granule(sg.tm_off, j * 8 + 2 * half + sl, r)) = i32x4{(int)hw[0], (int)hw[1], (int)hw[2], (int)hw[3]};
        const int byte = mx6_block_byte(amax);
        unsigned c[16], pw[3];
#pragma unroll
        for (int e = 0; e < 16; ++e) c[e] = mx6_code(val[e], byte);
        mx6_pack16(c, pw);
        // plane sl: dwords 0-3 in granule 4 + 2 sl, dwords 4-5 in granule 5 at byte 8 sl; this lane holds dwords 3 half .. 3 half + 2
        unsigned char *ga = oblk + (unsigned)mx_tm_granule(sg.tm_off, j * 8 + 4 + 2 * sl, r), *g5 = oblk + (unsigned)mx_tm_granule(sg.tm_off, j * 8 + 5, r) + 8 * sl;
        if (half == 0) {
            *reinterpret_cast<unsigned *>(ga + 0) = pw[0]; *reinterpret_cast<unsigned *>(ga + 4) = pw[1]; *reinterpret_cast<unsigned *>(ga + 8) = pw[2];
            (oblk + (unsigned)mx_tm_granule(sg.tm_off, 7, r))[8 * sl + j] = (unsigned char)byte;
        } else {
            *reinterpret_cast<unsigned *>(ga + 12) = pw[0]; *reinterpret_cast<unsigned *>(g5 + 0) = pw[1]; *reinterpret_cast<unsigned *>(g5 + 4) = pw[2];
        }
    }
}

}  // namespace jlm_mx
