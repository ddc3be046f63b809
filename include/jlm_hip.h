/*
 * jlm_hip.h -- C ABI of libjlm_hip.so, the MI355X (gfx950) implementation of
 * JLM's LSTM inference + lattice beam-search hot path.
 *
 * The reference has no FFI of its own: the path is pure Python over numpy
 * (decoder/model.py, decoder/decoder.py, decoder/decoder_dynamic.py).  Each
 * entry point below therefore replaces a group of numpy / Python statements of
 * the reference, cited as file:line.  The Python classes in jlm_amd/ keep the
 * reference's signatures and call these through ctypes (INTEGRATION.md shows
 * the binding a maintainer of the reference would add).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HBM) unless its name ends in _host;
 *   - `stream` is a hipStream_t passed as void*; calls only enqueue work;
 *   - return value: 0 on success, otherwise the hipError_t of the failed call
 *     (or -1 for an argument the kernels cannot handle, e.g. K % 4 != 0);
 *   - matrices are float32, row-major, leading dimension in floats, a multiple
 *     of 4, base pointers 16-byte aligned; scores are float64;
 *   - "rows" are beam hypotheses.  A hypothesis lives in global row
 *         g = frame * rmax + sentence * beam + slot,  rmax = nsent * beam,
 *     and all per-hypothesis arrays (score, lse, bp, node, word, h, c, T) are
 *     indexed by g.  `live` lists (compact r -> g) name the rows a frame steps.
 *   - counts that exist only on the device (number of live rows of a frame)
 *     are passed as `const int *n_dev`; kernels launched for the static upper
 *     bound exit early past *n_dev.
 */
#ifndef JLM_HIP_H
#define JLM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Library / device probe.  Returns the ABI version (JLM_ABI_VERSION). */
#define JLM_ABI_VERSION 12
#define JLM_MAX_BEAM 1024           /* ABI 6: jlm_beam_step takes beams above one wave (64): a lane owns several ranks */
int jlm_abi_version(void);
/* Writes gfx arch name (e.g. "gfx950:sramecc+:xnack-") of device `dev`. */
int jlm_device_arch(int dev, char *buf, int buflen);

/* ------------------------------------------------------------------------
 * K1+K2+K3+K9: embedding gather, fused gate GEMM, sigmoid/tanh, state update.
 * Replaces LSTM_Model._lstm_cell (decoder/model.py:125-139) and the state
 * gather/scatter of Decoder._batch_predict (decoder/decoder.py:206-218).
 *
 * For compact row r < min(n_rows_max, *n_dev):   g = rows ? rows[r] : r
 *   p = prev[g] (row whose state is consumed; <0 means zero state)
 *   x = [ h[p, 0:H] | emb[word[g], 0:E] ]
 *   z = x . Wt^T + bias     Wt is the packed [4H, kpad] gate matrix
 *   c[g] = c[p]*sig(z_f) + tanh(z_g)*sig(z_i) ;  h[g] = tanh(c[g])*sig(z_o)
 * Packed gate layout (jlm_amd/model.py packs it): row n of Wt / bias is
 *   n = (u / 16) * 64 + gate * 16 + (u % 16), gate order i,f,o,g
 * with Wt[n, 0:H] = HM_gate[:, u], Wt[n, H:H+E] = IM_gate[:, u], zero padded to
 * kpad (multiple of 32).  Requires H % 32 == 0, E % 4 == 0.
 */
int jlm_lstm_step(const float *h_in, const float *c_in, int ld_state,
                  float *h_out, float *c_out,
                  const int *rows, const int *prev, const int *word,
                  const float *emb, int ld_emb,
                  const float *wt, const float *bias, int kpad,
                  int H, int E, int n_rows_max, const int *n_dev, void *stream);

/* ------------------------------------------------------------------------
 * K4 / generic NT GEMM with optional row gathers and column bias:
 *   C[c_rows[m], n] = sum_k A[a_rows[m], k] * B[b_rows[n], k] + bias[n]
 * Replaces np.dot(hidden, PM) (model.py:145,162,184,186), the V_table
 * projections np.dot(temp, VT.T) (model.py:175,177) and, with b_rows = vocab,
 * the materialised logits of LSTM_Model.project (model.py:141-193).
 * NULL row maps mean identity; bias may be NULL.  K % 4 == 0.
 */
int jlm_gemm_nt(const float *A, int lda, const int *a_rows,
                const float *B, int ldb, const int *b_rows,
                float *C, int ldc, const int *c_rows, const float *bias,
                int M, int N, int K, const int *m_dev, void *stream);

/* ------------------------------------------------------------------------
 * K5+K6 fused: one vocabulary segment's logits are produced tile by tile on
 * the MFMA pipe and reduced on the fly to per-row (max, sum exp) partials; the
 * [rows, V] logits never reach HBM.  Replaces the full-vocabulary branch of
 * LSTM_Model.project + softmax (model.py:141-193,15-20).
 *   logit[v, r] = sum_k Bseg[v, k] * T[rows[r], k] + bias[v]   v < n_vocab
 *   part[(tile0 + v/128) * ld_part + r] = (max_v, sum_v exp(logit - max)) over the tile
 * Returns the number of vocab tiles used (>=0) or a negative error.
 */
int jlm_vocab_lse_partials(const float *Bseg, int ldb, int n_vocab, int K,
                           const float *T, int ldt, const int *rows,
                           const float *bias, float *part, int ld_part, int tile0,
                           int n_rows_max, const int *n_dev, void *stream);
/* lse[g] = log sum exp over n_tiles partials, float64;  g = rows[r]. */
int jlm_lse_combine(const float *part, int ld_part, int n_tiles,
                    const int *rows, double *lse,
                    int n_rows_max, const int *n_dev, void *stream);

/* ------------------------------------------------------------------------
 * Vocabulary segments for word-addressed logits (tied softmax: one segment;
 * D-softmax / D-softmax*: model.py:144-181).  Host struct, copied per call.
 */
typedef struct {
    int v_start, v_end;      /* word ids [v_start, v_end) */
    int k;                   /* contraction length (multiple of 4 after padding) */
    int t_off;               /* column offset of this segment's input inside T */
    const float *B;          /* [v_end - v_start, ldb] block, device */
    int ldb;
} jlm_segment;
#define JLM_MAX_SEGMENTS 8

/* Same reduction, rows-stationary form (the one the decoders use): all segments
 * of the model in ONE launch; a workgroup keeps 128 hypothesis rows' MFMA
 * fragments in registers and streams a range of vocabulary tiles past them, so
 * each row gets one (max, sum exp) partial per vocabulary RANGE:
 *   part[p * ld_part + r],  p < return value  (<= max_parts, <= 96)
 * Needs every segment's k <= 256; returns -2 otherwise (use the tile form).
 * Returns the number of partial slices (fold them with jlm_lse_combine) or <0. */
int jlm_vocab_lse_stationary(const jlm_segment *segs_host, int n_segs, const float *b2,
                             const float *T, int ldt, const int *rows,
                             float *part, int ld_part, int max_parts,
                             int n_rows_max, const int *n_dev, void *stream);

/* ------------------------------------------------------------------------
 * Split-f16 ("f16x3") operands.  The f32 matrix pipe of gfx950 runs at 1/16 of
 * the f16 rate; these entry points carry every f32 value x as two f16 halves
 *   x * scale = hi + lo (+ r, |r| <= 2^-22 |x * scale|)
 * and form a product as hi.hi + hi.lo + lo.hi in three f16 MFMAs with f32
 * accumulation -- f32-grade results (error pinned in tests/test_gpu_kernels.py)
 * at 16/3 of the f32 MFMA rate.  "Split rows": a row of k values, k padded with
 * zeros to a multiple of 16, stored as k/8 blocks of [8 x f16 hi][8 x f16 lo]
 * (4 bytes per value, row stride ld_dst in 4-byte units, a multiple of 16).
 * scale must be a power of two (so that dividing it out again is exact) chosen
 * so that max|x| * scale stays below 65504.  jlm_pack_split_f16 writes the
 * blocks that cover k rounded up to 16 values (zero padded) and leaves the rest
 * of each destination row alone, so a matrix can be packed in column ranges
 * with different scales (dst / src advanced by a multiple of 16 values).
 * The format, to the bit (tests/operand_cases.py split_pair; every writer is held
 * to it byte for byte by tests/test_gpu_operand_formats.py):
 *   x  = f32(src * scale)   ONE f32 rounding of the product (none for a power of two)
 *   hi = f16(x)             round to nearest even; f16 subnormals are kept
 *   lo = f16(x - hi)        x - hi is exact in f32; lo is taken against THIS hi
 * for every writer of split rows: this packer, jlm_pack_split_f16_col and the
 * split-row epilogue of the LSTM step (x = h' * h_scale; with the f32 copy of
 * h' requested, the split rows are exactly the split of that copy).  hi is never
 * rounded from the exact product while lo is taken from the f32 one: the launcher
 * also takes scales that are no power of two, and there the two would disagree
 * about hi on every f16 rounding tie of x.  A finite x gives finite halves with
 * |lo| <= ulp(hi) / 2 and f16(hi + lo) == hi -- but where a residual within 2^-12
 * of half an ulp rounds up to exactly that half ulp under an odd hi (a tie).
 * Written: the blocks covering k rounded up to 16 values, columns k .. zero;
 * nothing else. */
int jlm_pack_split_f16(const float *src, int rows, int k, int ld, float scale,
                       void *dst, int ld_dst, void *stream);

/* ABI 4: k-means compressed weights (train/comp.py:52-80; selected by decoder/model.py:74-78 through `comp`): per tensor a
 * uint8 code array and a float32 codebook of <= 256 entries.  dst[r][c] = codebook[code[r][c]] for c < k, on the device
 * (what np.take(codebook, code) does on the host in train/comp.py:70): the codes stay resident, the float panel is
 * expanded from them where the kernels need it.  Codebook entries are copied bit for bit (-0.0, subnormals, inf, NaN
 * payloads); a code >= n_codes gives +0.0 (the kernel's table of 256 entries is zero-filled behind the book), never a read past the
 * book.  Columns k .. ld_dst of a destination row are left alone. */
int jlm_dequant_u8(const uint8_t *code, int rows, int k, int ld_code, const float *codebook, int n_codes,
                   float *dst, int ld_dst, void *stream);

/* ABI 4: the decode's LSTM step (K1+K2+K3+K9; decoder/model.py:125-139 with the state gather / scatter of
 * Decoder._batch_predict, decoder/decoder.py:206-218), table form, one 160-row x 128-gate-column tile per CU.
 * Same row semantics as jlm_lstm_step.  Operands:
 *   h_in / h_out   split rows of the state scaled by h_scale (|h| < 1, h_scale a power of two <= 2^14);
 *   wt8            split rows [4H, H] of the state half of the gate matrix scaled by 1 / (descale * h_scale),
 *                  in the gate-interleave-8 row order  n = (u / 8) * 32 + gate * 8 + (u % 8), gate order i,f,o,g
 *                  (a 32-row MFMA block = four gates of eight units: the cell update needs no transposition);
 *   xgate8         f32 [V, 4H], same column order: (emb[w] . W_x^T + bias) / descale for every vocabulary word
 *                  (model.py:125-131 computes x.IM_g + h.HM_g + b_g; the table is the x.IM_g + b_g part);
 *   h_f32_out      optional (may be NULL): h' also as plain f32 rows, same stride (untied models: T is the state itself and
 *                  the edge-logit / word-list kernels read T as f32);
 *   c stays f32.   H % 32 == 0, ld_state % 16 == 0.  State rows are addressed as 16-byte records through a 31-bit index:
 *   (highest row number + 1) x ld_state / 4 < 2^31 (16.7 M rows at H = 512). */
int jlm_lstm_step_xg(const void *h_in, const float *c_in, int ld_state, void *h_out, float *c_out,
                     const int *rows, const int *prev, const int *word,
                     const void *wt8, const float *xgate8, int H, float descale, float h_scale, float *h_f32_out,
                     int n_rows_max, const int *n_dev, void *stream);

/* ABI 12: which kernel form jlm_lstm_step_xg launches for these arguments (pure host, no HIP call): 0 the loop for every H
 * (gate_xg_kernel), and at H = 512: 1 one 160 x 128 tile per workgroup (gate_xg_u16_kernel), 3 the same tile persistent (gate_pu_kernel),
 * 2 W-stationary persistent (gate_ws_kernel), 4 128 x 256 tiles persistent (gate_p2_kernel); -1 for an H the step refuses.
 * has_rows / has_h_f32: whether rows / h_f32_out are non-NULL.  Default by n_rows_max: 1 below 4 096, 3 up to 16 383, 2 from 16 384;
 * JLM_GATE_V = 1 .. 4 (read once per process) forces a form where it can serve the launch -- 2 and 3 need a row list, 4 a row list and
 * no f32 copy -- and the default is taken where it cannot. */
int jlm_lstm_step_form(int H, int has_rows, int has_h_f32, int n_rows_max);

/* jlm_vocab_lse_partials on split rows (the tile form for k > 256: untied models, k = H; model.py:189-191):
 *   logit[v, r] = descale * sum_k Bsplit[v, k] * Tsplit[rows[r], k] + bias[v]
 * Bsplit = split rows of the segment's matrix scaled by 2^eB, Tsplit = split rows of the row operand scaled by 2^eT (for an
 * untied model the state rows the LSTM step wrote, eT = 14), descale = 2^-(eT + eB); strides in 4-byte units, K % 16 == 0.
 * Same partial-slice contract and return value as jlm_vocab_lse_partials. */
int jlm_vocab_lse_partials_split(const void *Bsplit, int ldb, int n_vocab, int K, const void *Tsplit, int ldt, const int *rows,
                                 const float *bias, float descale, float *part, int ld_part, int tile0,
                                 int n_rows_max, const int *n_dev, void *stream);

/* jlm_gemm_nt on split rows: C = descale * (A . B^T) + bias, C plain f32. */
int jlm_gemm_nt_split(const void *A, int lda, const int *a_rows, const void *B, int ldb, const int *b_rows,
                      float *C, int ldc, const int *c_rows, const float *bias, float descale,
                      int M, int N, int K, const int *m_dev, void *stream);
/* ABI 12 (additive): which path jlm_gemm_nt_split takes for an M x N launch (pure host; the launcher asks here).  JLM_T_STAGES and
 * JLM_T_XCD are read once per process.  With JLM_T_STAGES = 3 (the default: the ring kernel, which since the chain-trips change keeps a
 * ring of four stages and two fragment register sets) and at most 256 tiles of 64 x 64:
 *   0 gemm_split3_kernel<Cfg64, ..., 4>, linear tile map (JLM_T_XCD=0)
 *   1 gemm_split3_kernel<Cfg64, ..., 4>, XCD map 1: the column tiles of a row tile on one XCD (default)
 * otherwise (any other JLM_T_STAGES: the two-stage kernel, same MFMA order, same bits) gemm_split_kernel, linear map:
 *   2 gemm_split_kernel<Cfg64>   fewer than 512 tiles of 128 x 128
 *   3 gemm_split_kernel<Cfg128>  the rest */
#define JLM_T_SPLIT3_LINEAR 0
#define JLM_T_SPLIT3_XCD 1
#define JLM_T_CFG64 2
#define JLM_T_CFG128 3
int jlm_gemm_nt_split_form(int M, int N);

/* One column of split rows from a vector: dst[r][col] = split(v[r] * scale) -- hi and lo as jlm_pack_split_f16 defines them, two f16
 * stores per row; the other 15 values of the touched 32-byte block and every other block are left alone. */
int jlm_pack_split_f16_col(const float *v, int rows, float scale, void *dst, int ld_dst, int col, void *stream);

/* jlm_vocab_lse_stationary on split rows: segs[i].B = split rows of the
 * segment's output embedding scaled by 2^eB_i, segs[i].ldb their stride in
 * 4-byte units, segs[i].k the true contraction length (<= 256, multiple of 4).
 * T is plain f32 (the kernel splits its rows while loading them, after scaling
 * by t_scale[i] = 2^eT_i); descale[i] = 2^-(eT_i + eB_i).
 * bias_col (may be NULL): bias_col[i] = segs[i].k says that column k of the
 * segment's split rows (the first padded one; needs k % 16 != 0) holds
 * b2[word] * 2^eB_i -- the kernel then feeds 1.0 at that position of every T
 * row and the bias costs nothing in the fold.  That 1.0 is scaled and split like
 * every T value: the column is multiplied by f32(t_scale log2 e) held as f16
 * hi + lo, which is log2(e) (1 + 6.9e-8) -- the same relative error on every
 * bias.  The packer of the column owes the correction (jlm_amd/rowformats.py
 * split_bias_correction; tests/test_gpu_split_logits.py pins it).
 * bias_col[i] = -1: b2 is added in the fold.  Same partial-slice contract and return value as
 * jlm_vocab_lse_stationary.  The vocabulary is cut into COLUMNS of equal cost
 * (one workgroup per column and 256-row tile), at most 256 / row tiles of them;
 * a column that crosses a segment boundary writes one slice per segment it
 * touches, so a launch writes at most columns + n_segs - 1 slices, and
 * max_parts (the capacity of `part` in slices) bounds the column count to
 * max_parts - (n_segs - 1). */
int jlm_vocab_lse_split(const jlm_segment *segs_host, const float *t_scale, const float *descale,
                        const int *bias_col, int n_segs, const float *b2,
                        const float *T, int ldt, const int *rows,
                        float *part, int ld_part, int max_parts,
                        int n_rows_max, const int *n_dev, void *stream);
/* ABI 12 (additive): the waves per workgroup of jlm_vocab_lse_split's kernel (pure host; the launcher asks here): 8
 * vocab_lse_split8_kernel (256 rows per workgroup, default), 4 vocab_lse_split_kernel (128 rows, two workgroups per CU;
 * JLM_LSE_WAVES=4, read once per process). */
int jlm_vocab_lse_split_form(void);

/* Word-list groups: one per (sentence, frame).  Group j covers hypothesis rows
 * g0[j] .. g0[j]+cnt[cnt_idx[j]]-1 and the word list number l = wl_base +
 * wl_idx[j], i.e. words wl[wl_off[l] .. wl_off[l+1]). */

/* K7 operand: logits of the lattice edges leaving a frame.  For every group j,
 * word position i in its list and beam slot k:
 *   edge[wl_out[i] * beam + k] = T[g0+k] . B[w_i] + b2[w_i]
 * (wl_out = lattice node id of the edge).  Replaces the indexing
 * pred[node.word_idx] of Path.append_node (decoder.py:43-49,172-182) -- only
 * the logits the lattice can consume are ever formed. */
int jlm_edge_logits(const jlm_segment *segs_host, int n_segs, const float *b2,
                    const float *T, int ldt,
                    const int *g0, const int *cnt, const int *cnt_idx,
                    const int *wl, const int *wl_off, const int *wl_idx, int wl_base,
                    const int *wl_out, float *edge, int beam, int n_groups, void *stream);

/* K5b/K6/K11: log-sum-exp over a selected vocabulary (vocab_select), or its
 * online extension by newly needed words (incremental vocabulary selection).
 * Replaces project(hidden, vocab)+softmax (model.py:184,15-20; decoder.py:202-218)
 * and the back-fill + re-softmax of DynamicDecoder._incremental_decode
 * (decoder_dynamic.py:133-148).  merge=0: (m,s) := over the list; merge=1:
 * (m,s) := (m,s) (+) list.  lse[g] = m + log(s) is refreshed either way.
 * Duplicate words in a list count twice, as in the reference. */
int jlm_wordlist_lse(const jlm_segment *segs_host, int n_segs, const float *b2,
                     const float *T, int ldt,
                     const int *g0, const int *cnt, const int *cnt_idx,
                     const int *wl, const int *wl_off, const int *wl_idx, int wl_base,
                     float *run_max, double *run_sum, double *lse,
                     int merge, int beam, int n_groups, void *stream);

/* jlm_edge_logits / jlm_wordlist_lse with the weight row and the bias of a list position taken from DIFFERENT words:
 * position i uses the weight row of word wl_w[i] and the bias of word wl[i] (wl_w == NULL: the plain forms).  This is
 * what the reference computes in DynamicDecoder on D-softmax / D-softmax* models, where project() returns the
 * columns of a vocabulary subset segment-major and the caller reads them in list order (model.py:152-158,168-179
 * under decoder_dynamic.py:130) -- reproduced behind DynamicDecoder.compat_quirks. */
int jlm_edge_logits_perm(const jlm_segment *segs_host, int n_segs, const float *b2,
                         const float *T, int ldt,
                         const int *g0, const int *cnt, const int *cnt_idx,
                         const int *wl, const int *wl_w, const int *wl_off, const int *wl_idx, int wl_base,
                         const int *wl_out, float *edge, int beam, int n_groups, void *stream);
int jlm_wordlist_lse_perm(const jlm_segment *segs_host, int n_segs, const float *b2,
                          const float *T, int ldt,
                          const int *g0, const int *cnt, const int *cnt_idx,
                          const int *wl, const int *wl_w, const int *wl_off, const int *wl_idx, int wl_base,
                          float *run_max, double *run_sum, double *lse,
                          int merge, int beam, int n_groups, void *stream);

/* jlm_wordlist_lse on split rows, single-segment models (seg->B = split rows scaled by 2^eB,
 * t_scale = 2^eT, descale = 2^-(eT+eB) as for jlm_vocab_lse_split; b2 is added in the fold).
 * max_words = longest word list among the groups (<= 4064; shorter lists run too when called here).  Returns -2 when
 * the shape is outside the kernel (k > 256, beam > 64, longer lists; jlm_wordlist_lse_form): use jlm_wordlist_lse then. */
int jlm_wordlist_lse_split(const jlm_segment *seg_host, float t_scale, float descale, const float *b2,
                           const float *T, int ldt,
                           const int *g0, const int *cnt, const int *cnt_idx,
                           const int *wl, const int *wl_off, const int *wl_idx, int wl_base, int max_words,
                           float *run_max, double *run_sum, double *lse,
                           int merge, int beam, int n_groups, void *stream);

/* K11 for a whole frame in one launch (DynamicDecoder._incremental_decode, decoder_dynamic.py:133-148):
 * every row g = fr * rmax + s * beam + slot, fr < n_old_frames, slot < cnt[fr * n_sent + s], of every
 * sentence s merges the words wl[wl_off[wl_base + s] .. wl_off[wl_base + s + 1]) into its running
 * (run_max, run_sum) and refreshes lse -- what jlm_wordlist_lse(merge = 1) does for n_old_frames * n_sent
 * groups, but with one workgroup per sentence gathering the list once.  rmax = n_sent * beam.
 * Returns -2 outside the kernel's shape (max_words > 128, k > 256, beam > 64; jlm_wordlist_merge_form). */
int jlm_wordlist_merge_split(const jlm_segment *seg_host, float t_scale, float descale, const float *b2,
                             const float *T, int ldt, const int *cnt, int n_sent, int beam, int n_old_frames,
                             const int *wl, const int *wl_off, int wl_base, int max_words,
                             float *run_max, double *run_sum, double *lse, void *stream);

/* ABI 12 (additive): which kernel the word-list normaliser launches (pure host, no HIP call).  jlm_decode_frames,
 * jlm_wordlist_lse(_perm), jlm_wordlist_lse_split and jlm_wordlist_merge_split ask here and decide nowhere else.
 * segs_host / n_segs: the f32 segments; split_seg: the split rows of a single-segment model (NULL: none); has_wl_w:
 * whether a weight-word list is given (the *_perm entry points); max_words: the longest list of the launch.
 * JLM_WORDLIST_MFMA (read once per process; 0 switches the matrix-pipe form off) is the only setting.
 *   0 JLM_WL_F32          wordlist_kernel<1> (csrc/jlm_beam.hip): any segments, any k, any beam, weight-word lists
 *   1 JLM_WL_MFMA         wordlist_lse_mfma_kernel<NK> (csrc/jlm_gemm.hip), NK = ceil(k / 32): one f32 segment,
 *                         1 <= k <= 256, beam <= 64, no weight-word list, JLM_WORDLIST_MFMA unset or non-zero
 *   2 JLM_WL_SPLIT        wordlist_lse_split_kernel<NS> (csrc/jlm_split.hip), NS = 2 / 4 / 8 / 12 / 16 for ceil(k / 16)
 *                         up to that: split rows, one segment, beam <= 64, 128 <= max_words <= 4064, no weight-word list
 *   3 JLM_WL_MERGE_SPLIT  wordlist_merge_split_kernel<NS> (csrc/jlm_split.hip), NS = 4 / 8 / 12 / 16: the incremental
 *                         back-fill on split rows, one segment, beam <= 64, max_words <= 128
 * jlm_wordlist_lse_form returns 0, 1 or 2, or -1 for segments the f32 kernels refuse (bad count, k / ldb / t_off / ldt
 * not multiples of 4, rows past LDS).  jlm_wordlist_merge_form returns 3, or else the group-wise merge through
 * jlm_wordlist_lse(_split) with merge = 1: what jlm_wordlist_lse_form(segs, n, split_seg, 0, ...) returns. */
#define JLM_WL_F32 0
#define JLM_WL_MFMA 1
#define JLM_WL_SPLIT 2
#define JLM_WL_MERGE_SPLIT 3
#define JLM_WL_SPLIT_MIN_WORDS 128
#define JLM_WL_SPLIT_MAX_WORDS 4064
#define JLM_WL_MERGE_MAX_WORDS 128
int jlm_wordlist_lse_form(const jlm_segment *segs_host, int n_segs, const jlm_segment *split_seg, int has_wl_w, int ldt,
                          int beam, int max_words);
int jlm_wordlist_merge_form(const jlm_segment *segs_host, int n_segs, const jlm_segment *split_seg, int ldt, int beam,
                            int max_words);

/* ------------------------------------------------------------------------
 * Lattice of a batch (CSR, built on the host by jlm_amd/lattice.py following
 * Decoder._build_lattice, decoder.py:79-135), resident in HBM for the decode.
 */
typedef struct {
    int n_sent, beam, n_frames;   /* n_frames = max sentence length + 1 */
    const int *sent_len;          /* [n_sent] kana length */
    const int *end_off;           /* [n_frames*n_sent + 1] nodes ending at (frame, sentence) */
    const int *node_start;        /* [n_nodes] start frame (-1 for <eos>) */
    const int *node_word;         /* [n_nodes] softmax row of the word */
} jlm_lattice;

typedef struct {
    double *score;                /* [G] accumulated -log p (decoder.py:36,49) */
    double *lse;                  /* [G] log-normaliser of the row's next-word distribution */
    double *ysum;                 /* [G] dynamic decoder: sum of edge logits along the path */
    int *bp;                      /* [G] previous hypothesis row (-1 at the root) */
    int *node;                    /* [G] lattice node consumed last */
    int *word;                    /* [G] its softmax row (LSTM input) */
    int *cnt;                     /* [n_frames*n_sent] hypotheses alive per (frame, sentence) */
    int *live;                    /* [n_frames*rmax] compact list of rows to step per frame */
    int *n_live;                  /* [n_frames] */
    const float *edge;            /* [n_nodes*beam] edge logits */
    /* -- ABI 2: fused K6 tail.  live_base[(frame, sentence)] = position of the sentence's first row
     * in live[frame] (written by jlm_beam_step when it lists the rows; may be NULL).  lse_part != NULL
     * (mode 0 only): the n_parts partial slices [n_parts][ld_part] of (max, sum exp) pairs that
     * jlm_vocab_lse_* left for the rows of frame - 1, indexed by live position, are folded into
     * lse[] by jlm_beam_step(frame) itself -- no jlm_lse_combine launch in between. */
    int *live_base;               /* [n_frames*n_sent] */
    const float *lse_part;
    int ld_part, n_parts;
    /* ABI 11: one device int (NULL: none) that jlm_beam_step ORs 1 into when a folded log-normaliser is not finite -- a row whose
     * logits left the range of the fixed-reference normaliser (jlm_vocab_lse_mixed_fr: sum 2^y overflowed to inf or vanished to 0).
     * An overflowed row's hypotheses score -inf and are pruned silently otherwise; the caller zeroes the int per batch and reads it
     * back with the traces (jlm_amd/engine.py: DecodeEngine.collect raises). */
    int *flags;
} jlm_beam_state;

/* K7+K8: candidate scoring and stable per-sentence top-k for frame `frame`.
 * Replaces Decoder._build_current_frame + sort/truncate (decoder.py:164-182,
 * 227-229).  mode 0: static decoder, score = score[p] + lse[p] - edge;
 * mode 1: self-normalised model, score = score[p] - edge (model.py:117-118);
 * mode 2: DynamicDecoder (decoder_dynamic.py:53-91,150-175): every path is
 * re-scored from the head with the current normalisers.
 * Ties keep candidate generation order (node order, then beam slot).  Rows of
 * a sentence's last frame are not listed in `live`: the reference steps them
 * too but never reads the result (decoder.py:233-237).
 * max_cands >= beam * (largest number of nodes ending at one (frame, sentence)).
 * 1 <= beam <= JLM_MAX_BEAM (the reference has no limit, decoder.py:227-229); a cell's candidates live in one wave's
 * LDS -- in one piece up to ~13 k, above that chunk by chunk with the chunks' winners merged (round 6: same order, same result);
 * -1 when max_cands exceeds jlm_beam_step_max_cands(beam, n_frames, mode), and for a state of more than 2^29 rows
 * (n_frames x n_sent x beam) in the one-piece form, whose kernel addresses score / lse / ysum rows by 32-bit byte offsets.
 * Every cell at frame <= sent_len holds at least one node: the real lattice always has the raw-kana fallback, so an empty cell
 * is not a case (the kernels clamp a lane's candidate to C - 1 and assume C >= 1). */
int jlm_beam_step(const jlm_lattice *lat_host, const jlm_beam_state *st_host,
                  int frame, int mode, int max_cands, void *stream);

/* ABI 12 (additive): which kernel jlm_beam_step / jlm_backtrace launches for a shape (pure host, no HIP call; the launchers ask
 * here and decide nowhere else).  JLM_BEAM_CHUNK=<candidates> (every launch through the chunked kernel with that chunk size) and
 * JLM_BACKTRACE_WAVE=0 (the thread-per-path kernel for every shape) are read once per process and take part.
 *   0 JLM_BEAM_STEP_ONE_PIECE  beam_step_kernel<mode>: the cell's keys in one wave's LDS (max_cands up to ~13 k at beam 10)
 *   1 JLM_BEAM_STEP_CHUNKED    beam_step_chunked_kernel<mode>: chunk by chunk, then a selection over the chunk winners
 * jlm_beam_step_form returns -1 where jlm_beam_step refuses the shape (beam, n_frames or mode out of range; chunk winners past LDS).
 *   0 JLM_BACKTRACE_WAVE4      backtrace_wave_kernel<4>:  beam <= 64, n_frames x beam <= 256
 *   1 JLM_BACKTRACE_WAVE8      backtrace_wave_kernel<8>:  beam <= 64, n_frames x beam <= 512
 *   2 JLM_BACKTRACE_WAVE16     backtrace_wave_kernel<16>: beam <= 64, n_frames x beam <= 1024
 *   3 JLM_BACKTRACE_THREAD     backtrace_kernel (a thread per path): every other shape */
#define JLM_BEAM_STEP_ONE_PIECE 0
#define JLM_BEAM_STEP_CHUNKED 1
#define JLM_BACKTRACE_WAVE4 0
#define JLM_BACKTRACE_WAVE8 1
#define JLM_BACKTRACE_WAVE16 2
#define JLM_BACKTRACE_THREAD 3
int jlm_beam_step_form(int beam, int n_frames, int mode, int max_cands);
int jlm_backtrace_form(int beam, int n_frames);

/* ABI 7: the vocabulary projection + log-sum-exp with the two cross terms of the split product on the INT8 matrix pipe
 * (csrc/jlm_mixed.hip; reference project + softmax, decoder/model.py:141-193, 15-20).
 *   t.b ~ t_hi.b_hi (f16 x f16, v_mfma_f32_32x32x16_f16) + [t_hi.b_lo + t_lo.b_hi] (int8 x int8 into one i32 accumulator,
 *         v_mfma_i32_32x32x32_i8; hi8 = rint(hi / s), lo8 = rint(lo / (s 2^-11)), s a power of two per T row / per segment)
 * "Mixed rows": per 32 k-values a 128-byte block [32 x f16 hi | 32 x int8 hi8 | 32 x int8 lo8]; the bias of a word rides in
 * the f16 part as columns k (hi of b2 2^eB log2 e) and k + 1 (its f16 residual x 2^11), so a row has nb = ceil((k + 2) / 32)
 * blocks (ld_dst = 32 nb in 4-byte units, nb <= 8) -- or, for k a multiple of 32, nb = k / 32 and no bias columns (below).
 * jlm_pack_mixed: src [rows, k] f32 (stride ld) and bias [rows] -> dst; scale = 2^eB, bias_scale = 2^eB log2 e, s8 = the
 * segment's int8 scale (a power of two >= max |f16(src scale)| / 127).  k is a multiple of 4 (-1 otherwise).
 * The format, to the bit (tests/operand_cases.py mixed_row_bytes / t_row_bytes; tests/test_gpu_operand_formats.py):
 *   vocabulary rows   x = f32(src scale) (exact: a power of two), hi = f16(x), lo = x - hi (f32, not rounded to f16);
 *                     hi8 = rint(hi / s8), lo8 = rint(lo / (s8 / 2048)): ties to even, then clipped to +-127; zero behind k.
 *                     Bias columns: xb = f32(bias bias_scale) (one f32 rounding), column k = f16(xb), column k + 1 =
 *                     f16((xb - f16(xb)) 2048), zeros for bias = NULL; the f16 columns behind them zero.  Every byte of a row's nb
 *                     blocks is written.
 *   hypothesis rows   m = f32(2^eT log2 e).  hi = f16 of the EXACT product T m -- ONE rounding (v_fma_mixlo_f16), not f16(f32(T m)) --;
 *                     the row's scale per segment s = the smallest power of two >= max |hi| / 127 over the segment's k values
 *                     ((bits(f32(max / 127)) + 0x007fffff) & 0x7f800000; 1.0 for an all-zero segment), hi8 = rint(hi / s),
 *                     lo8 = rint((f32(T m) - hi) / (s / 2048)), ties to even, clipped to +-127, zero behind k.  Written: every byte
 *                     of the blocks of rows below min(*n_dev, n_rows_max) and float i < n_segs of their JLM_MAX_SEGMENTS scale
 *                     floats; the other scale floats, the rows from there on and the rest of the last 32-row block are left alone. */
int jlm_pack_mixed(const float *src, int rows, int k, int ld, const float *bias, float scale, float bias_scale, float s8,
                   void *dst, int ld_dst, void *stream);
/* The hypothesis side: T [G, ldt] f32 -> packed rows Tm, COMPACT: packed row r = hypothesis row rows[r] (a frame's live rows: one
 * small buffer, rewritten every frame) (ld_tm = jlm_mixed_t_stride(segs, n_segs), 4-byte units per row): per segment nb blocks of
 * x = T 2^eT log2 e in the same block format, the bias constants 2^eT / 2^(eT-11) at columns k, k + 1 of the f16 part, and
 * JLM_MAX_SEGMENTS floats per row: the row's int8 scale per segment.  Once per row and frame (one wave per row); the vocabulary
 * kernel's workgroups only load the result.  t_scale[i] = 2^eT_i (a power of two).
 * ABI 9: the buffer is an opaque image of WHOLE 32-row blocks -- the caller allocates ceil(n_rows_max / 32) * 32 rows of ld_tm
 * floats -- laid out granule-major inside a block (16-byte granule g of row r at block (r / 32) + g * 512 + (r % 32) * 16, the
 * scales behind the granules), so that a wave of the vocabulary kernel reads one contiguous kilobyte per operand load. */
int jlm_mixed_t_stride(const jlm_segment *segs_host, int n_segs);
int jlm_pack_t_mixed(const jlm_segment *segs_host, const float *t_scale, int n_segs, const float *T, int ldt, const int *rows,
                     int n_rows_max, const int *n_dev, void *Tm, int ld_tm, void *stream);
/* ABI 11 (round 6): mx6 rows -- the two cross terms of the split product as FP6 (e2m3) x FP6 on the block-scaled matrix instruction
 * (v_mfma_scale_f32_32x32x64_f8f6f4: one instruction per 32 k-values for both terms, accumulated into the f16 pass's f32 accumulator;
 * csrc/jlm_mx6_body.h, csrc/jlm_mx6.hip; reference project + softmax, decoder/model.py:141-193, 15-20).  Same 128-byte blocks, strides
 * and buffers as the int8 form; granules 4-6 of a block hold the FP6 planes (hi6, lo6) and granule 7 of a row's first block their E8M0
 * scales, one per plane and 32 k-values.  The f16 plane of BOTH mx6 packers is f16(f32(x scale)) -- two roundings, where the int8
 * hypothesis-row packer has one --, the FP6 planes are those of that hi and of f32(x scale) - hi over the real k-values: nearest e2m3
 * value, ties to even, saturating at 7.5, against the smallest power of two s with max <= 7.5 s per plane and block (byte 0 for an all-zero
 * block).  Vocabulary rows: half 0 = hi6, half 1 = lo6, every byte of a row written (granule 7 zero but for the scale bytes j / 8 + j of
 * block j in the row's first block).  Hypothesis rows: the halves swapped; of granule 7 only the scale bytes j / 8 + j (j < nb) of a
 * segment's first block are written -- the rest of that granule, granule 7 of the other blocks and the row's scale floats are left alone.
 * Selected by s8 = 0:
 *   jlm_pack_mixed(..., s8 = 0, ...)           packs a vocabulary block as mx6 rows (at most 8 blocks per row: k + 2 <= 256 or k = 256);
 *   jlm_pack_t_mixed6                            packs hypothesis rows in that form (same arguments and stride as jlm_pack_t_mixed);
 *   jlm_vocab_lse_mixed(_fr)(..., s8[i] = 0 for EVERY segment, ...)  runs the launch on mx6 rows (-2: formats mixed within a launch,
 *                                                or k = 512); jlm_vocab_lse_hybrid takes int8 rows only (-2);
 *   jlm_decode_model.mixed_s8[i] = 0 for every mixed segment makes jlm_decode_frames / jlm_lse_probe use the two above. */
int jlm_pack_t_mixed6(const jlm_segment *segs_host, const float *t_scale, int n_segs, const float *T, int ldt, const int *rows,
                      int n_rows_max, const int *n_dev, void *Tm, int ld_tm, void *stream);
/* ABI 12 (additive): the tail of a decode frame between the T projection and the normaliser as ONE launch (csrc/jlm_frame_tail.hip) --
 * jlm_pack_t_mixed6 of the frame's live rows and jlm_edge_logits of its cells, to the bit.  One workgroup per cell j < n_groups of
 * frame `frame` (cell j is sentence j: g0, cnt_idx, wl_idx, sent_len and live_base are indexed by j, so the caller passes the frame's
 * slices): it stages the cell's rows T[g0[j] .. + min(cnt[cnt_idx[j]], beam)) in LDS once, writes edge[] for the words of list
 * wl_base + wl_idx[j] like jlm_edge_logits, and -- when frame < sent_len[j], i.e. the rows are in the frame's live list -- packs row
 * g0[j] + slot into Tm at the compact row live_base[j] + slot (what beam_step_kernel recorded), like jlm_pack_t_mixed6 over that list.
 * segs: the f32 segments of the edge logits; mixed_segs / t_scale / n_mixed / ld_tm: as jlm_pack_t_mixed6.
 * -2: a shape the kernel does not host (beam > 16, k > 256, more than 8 blocks in a segment, more than 32 KB of LDS): the caller
 * launches the two kernels.  jlm_pack_edge_mx6_lds_bytes: the launch's LDS at row stride ldt (pure host; -1: ldt not a multiple of 4). */
int jlm_pack_edge_mx6(const jlm_segment *segs_host, int n_segs, const float *b2, const jlm_segment *mixed_segs, const float *t_scale,
                      int n_mixed, const float *T, int ldt, const int *g0, const int *cnt, const int *cnt_idx, const int *wl,
                      const int *wl_off, const int *wl_idx, int wl_base, const int *wl_out, float *edge, int beam, int n_groups,
                      const int *sent_len, const int *live_base, int frame, void *Tm, int ld_tm, void *stream);
int jlm_pack_edge_mx6_lds_bytes(int ldt);
/* segs[i].B = mixed rows, segs[i].ldb = 32 nb, segs[i].k the true contraction length; descale[i] = 2^-(eT_i + eB_i), s8[i] as
 * above; Tm = the packed hypothesis rows.  Same partial-slice contract and return value as jlm_vocab_lse_split; -2: a shape
 * this form does not take (more than 8 blocks; segments of both bias forms in one launch).
 * A contraction that fills its last block (k a multiple of 32: the tied k = 256 models) has no columns left for the bias: its
 * rows are packed with ld_dst = k (jlm_pack_mixed then ignores `bias`), segs[i].ldb = k says so, and the kernel takes the
 * biases from bias2 [V] = b2 log2(e) (device; may be NULL otherwise) -- staged into LDS beside each tile, added in the combine. */
int jlm_vocab_lse_mixed(const jlm_segment *segs_host, const float *descale, const float *s8, const float *bias2, int n_segs,
                        const void *Tm, int ld_tm, float *part, int ld_part, int max_parts, int n_rows_max,
                        const int *n_dev, void *stream);
/* ABI 9: the same launch WITHOUT a running maximum where a kernel form for it exists (the wide kernel's tied k = 256 and k = 512 forms;
 * every other shape runs exactly as jlm_vocab_lse_mixed): s = sum over the words of 2^(base-2 logit) against the fixed reference 0, slices
 * (0, s) -- three VALU instructions per logit less.  Valid while every row's largest logit stays within about +-69 (base-2: +-100: f32
 * range over 2^16 words); a row outside it comes back as s = 0 or inf.  The caller decides per model (jlm_decode_model.lse_fixed_ref). */
int jlm_vocab_lse_mixed_fr(const jlm_segment *segs_host, const float *descale, const float *s8, const float *bias2, int n_segs,
                        const void *Tm, int ld_tm, float *part, int ld_part, int max_parts, int n_rows_max,
                        const int *n_dev, void *stream);

/* ABI 12 (additive): which kernel jlm_vocab_lse_mixed (fixed_ref = 0) / jlm_vocab_lse_mixed_fr (fixed_ref = 1) launches for these
 * segments (pure host, no HIP call; the launchers ask here).  has_bias2: whether bias2 is non-NULL.  -1 / -2 exactly when the launcher
 * refuses the segments (bad count; a shape no form hosts, formats or bias forms mixed within a launch, mx6 rows at k = 512); the
 * launcher's other refusals (ld_tm, n_rows_max, max_parts) do not depend on the form.  JLM_MX_WIDE and JLM_MX6_WIDE are read once per
 * process.  int8 planes (csrc/jlm_mixed.hip: eight waves, 256 rows per workgroup; csrc/jlm_mixed_w.hip: the wide kernel, four waves):
 *    0 MX_KERNEL_DSOFTMAX       vocab_lse_mixed_kernel<true, false, 7, 13, 4, 7, 2, 4>   the D-softmax* 200 / 100 / 50 shapes
 *    1 MX_KERNEL_GENERIC        vocab_lse_mixed_kernel<false, false, ...>               every other bias-column shape
 *    2 MX_KERNEL_TIED           vocab_lse_mixed_kernel<true, true, 8, 16>               tied k = 256 under JLM_MX_WIDE=0
 *    3 MX_KERNEL_GENERIC_XB     vocab_lse_mixed_kernel<false, true, ...>                external-bias k = 64, 128, 192
 *    4 MXW_KERNEL_DSOFTMAX      vocab_lse_mixedw_kernel<2, false, false, ...>           the D-softmax* shapes under JLM_MX_WIDE=1
 *                                                                                        (ignores fixed_ref)
 *    5 MXW_KERNEL_K512          vocab_lse_mixedw_kernel<1, true, false, 16, 32>         one segment of k = 512, 128 rows per workgroup
 *    6 MXW_KERNEL_TIED          vocab_lse_mixedw_kernel<2, true, false, 8, 16>          tied k = 256 (default)
 *    7 MXW_KERNEL_K512_FR       vocab_lse_mixedw_kernel<1, true, true, 16, 32>          5 without a running maximum
 *    8 MXW_KERNEL_TIED_FR       vocab_lse_mixedw_kernel<2, true, true, 8, 16>           6 without a running maximum
 * mx6 planes (every s8[i] = 0; csrc/jlm_mx6.hip eight waves, csrc/jlm_mx6w.hip four waves; the _FR forms only where every descale is 1):
 *    9 MX6_KERNEL_DSOFTMAX      vocab_lse_mx6_kernel<true, false, false, ...>           the D-softmax* shapes (default)
 *   10 MX6_KERNEL_GENERIC       vocab_lse_mx6_kernel<false, false, false, ...>          every other bias-column shape
 *   11 MX6_KERNEL_TIED          vocab_lse_mx6_kernel<true, true, false, 8, 16>          tied k = 256 under JLM_MX6_WIDE=0
 *   12 MX6_KERNEL_GENERIC_XB    vocab_lse_mx6_kernel<false, true, false, ...>           external-bias k = 64, 128, 192
 *   13 MX6_KERNEL_DSOFTMAX_FR   vocab_lse_mx6_kernel<true, false, true, ...>            9 without a running maximum
 *   14 MX6_KERNEL_TIED_FR       vocab_lse_mx6_kernel<true, true, true, 8, 16>           11 without a running maximum
 *   15 MX6W_KERNEL_DSOFTMAX     vocab_lse_mx6w_kernel<false, false, ...>                the D-softmax* shapes under JLM_MX6_WIDE=1
 *   16 MX6W_KERNEL_DSOFTMAX_FR  vocab_lse_mx6w_kernel<false, true, ...>                 15 without a running maximum
 *   17 MX6W_KERNEL_TIED         vocab_lse_mx6w_kernel<true, false, 8, 16>               tied k = 256 (default)
 *   18 MX6W_KERNEL_TIED_FR      vocab_lse_mx6w_kernel<true, true, 8, 16>                17 without a running maximum */
#define JLM_LSE_MX_DSOFTMAX 0
#define JLM_LSE_MX_GENERIC 1
#define JLM_LSE_MX_TIED 2
#define JLM_LSE_MX_GENERIC_XB 3
#define JLM_LSE_MXW_DSOFTMAX 4
#define JLM_LSE_MXW_K512 5
#define JLM_LSE_MXW_TIED 6
#define JLM_LSE_MXW_K512_FR 7
#define JLM_LSE_MXW_TIED_FR 8
#define JLM_LSE_MX6_DSOFTMAX 9
#define JLM_LSE_MX6_GENERIC 10
#define JLM_LSE_MX6_TIED 11
#define JLM_LSE_MX6_GENERIC_XB 12
#define JLM_LSE_MX6_DSOFTMAX_FR 13
#define JLM_LSE_MX6_TIED_FR 14
#define JLM_LSE_MX6W_DSOFTMAX 15
#define JLM_LSE_MX6W_DSOFTMAX_FR 16
#define JLM_LSE_MX6W_TIED 17
#define JLM_LSE_MX6W_TIED_FR 18
int jlm_vocab_lse_mixed_form(const jlm_segment *segs_host, const float *descale, const float *s8, int has_bias2, int n_segs,
                             int fixed_ref);

/* One launch over segments of BOTH formats (csrc/jlm_split.hip, vocab_lse_hybrid_kernel): mixed[i].B != NULL runs segment i on
 * its mixed rows (mixed[i].ldb = 32 nb; mx_descale[i], mx_s8[i] as for jlm_vocab_lse_mixed; Tm = rows packed by
 * jlm_pack_t_mixed over the MIXED segments only, in segment order, for the same `rows`), the others on their split rows exactly as
 * jlm_vocab_lse_split (segs / t_scale / descale / bias_col cover every segment).  The int8 cross terms pay where the matrix
 * instructions dominate a block (k = 200, 100); where the fold does (k = 50) the three f16 passes stay.  -2: a shape the kernel
 * does not host (mixed: k + 2 in (192, 208], (96, 112] or (32, 64]; split: k <= 208, not a multiple of 16, with its bias column): use
 * jlm_vocab_lse_split.
 * ABI 10, head_split (host array of n_segs ints, or NULL): the first head_split[i] words of MIXED segment i (a multiple of 128, less
 * than the segment) run on its split rows, the rest on its mixed rows.  In a trained model the frequent words -- the low ids of the
 * first segment -- carry the probability mass and with it the int8 cross terms' contribution to the log-normaliser's error (measured
 * on logits of +-20: head segment 3.1e-6 rms, the other two 2e-8); three f16 passes for those few thousand words buy the split form's
 * accuracy at the mixed form's cost for the other 90 % of the vocabulary.  The loader picks the cut (DeviceModel._calibrate_mixed). */
int jlm_vocab_lse_hybrid(const jlm_segment *segs_host, const float *t_scale, const float *descale, const int *bias_col,
                         const jlm_segment *mixed, const float *mx_descale, const float *mx_s8, const int *head_split, int n_segs,
                         const float *b2, const float *T, int ldt, const void *Tm, int ld_tm, const int *rows, float *part, int ld_part,
                         int max_parts, int n_rows_max, const int *n_dev, void *stream);

/* ABI 6: the largest max_cands (a multiple of 256, as the plans round it) jlm_beam_step accepts for this beam,
 * frame count and mode -- the launcher's own LDS formula, so that callers can route sentences with a larger lattice
 * cell to a host-side search (Decoder._decode_unpruned / DynamicDecoder._decode_host) instead of failing the batch.
 * Round 6: cells that do not fit one wave's LDS in one piece are selected chunk by chunk, so the figure is what the chunk
 * winners leave room for (3.4 M candidates at beam 10, 0.5 M at beam 64): no real lexicon gets near it.
 * 0: no cell fits (beam or frame count too large).  Pure host function, no GPU needed. */
int jlm_beam_step_max_cands(int beam, int n_frames, int mode);

/* Additive (ABI 12): the dynamic LDS one launch asks for -- the launchers' own formulas -- so that the residency budget of the small
 * per-frame kernels beside a resident normaliser workgroup can be checked without a GPU.
 * jlm_beam_step_lds_bytes: jlm_beam_step's one-piece kernel for this beam, frame count, mode and max_cands; 0: bad arguments.
 * jlm_vocab_lse_mixed_lds_bytes: jlm_vocab_lse_mixed(_fr) for these segments (mixed or mx6 rows); -1 / -2: shapes it refuses.
 * Pure host functions. */
int jlm_beam_step_lds_bytes(int beam, int n_frames, int mode, int max_cands);
int jlm_vocab_lse_mixed_lds_bytes(const jlm_segment *segs_host, int n_segs);

/* K10: n-best read-out.  For sentence s and rank r < cnt at its last frame:
 * out_nodes[(s*beam+r)*stride + d] = node ids from the LAST word back to the
 * root, out_len = number of nodes, out_score = path score (decoder.py:237). */
int jlm_backtrace(const jlm_lattice *lat_host, const jlm_beam_state *st_host,
                  int *out_nodes, int *out_len, double *out_score, int stride, void *stream);

/* K6: row softmax / exp for the LSTM_Model.predict API (model.py:15-20,117-120).
 * pred[r, :] = self_norm ? exp(y[r, :]) : softmax(y[r, :]). */
int jlm_softmax_rows(const float *y, float *pred, int ld, int n_rows, int n_cols,
                     int self_norm, void *stream);

/* ------------------------------------------------------------------------
 * ABI 3: the frame loop itself.  Decoder.decode (decoder/decoder.py:220-241:
 * for every frame build the candidates, keep the best `beam`, step the LSTM of
 * the survivors) and DynamicDecoder.decode / _incremental_decode
 * (decoder/decoder_dynamic.py:177-194, 93-175) as ONE call that enqueues the
 * whole launch sequence of a batch -- per frame
 *   [incremental: merge the frame's new words into all older rows]  jlm_wordlist_merge_split | jlm_wordlist_lse(merge)
 *   jlm_beam_step                (folds the previous frame's normaliser slices)
 *   jlm_lstm_step_xg | jlm_lstm_step(_split), jlm_gemm_nt(_split) (T projection)
 *   jlm_edge_logits              (on `side_stream` when given, forked after T and joined before the next beam step)
 *   [jlm_pack_t_mixed +] jlm_vocab_lse_hybrid | jlm_vocab_lse_split | _stationary | jlm_wordlist_lse(_split)
 * and jlm_backtrace at the end -- exactly the calls a host would make one by
 * one through the entry points above (jlm_amd/engine.py does, for timing and
 * for models outside this call's shapes), without ~170 trips through the host
 * language's FFI per batch.  Nothing here synchronises with the device.
 */
typedef struct {
    const jlm_segment *segs;        /* f32 segments (edge logits, short word lists) */
    int n_segs;
    const float *b2;
    int H, ldt;
    int untied;                     /* T aliases h: no T projection (model.py:189-191) */
    int self_norm;                  /* no normaliser at all (model.py:117-118) */
    int split_lstm;                 /* state rows and gate matrix are split rows */
    /* jlm_lstm_step operands (split_lstm == 0) */
    const float *emb; int ld_emb; const float *wt; const float *gate_bias; int kpad, E;
    /* jlm_lstm_step_xg operands (split_lstm == 1; the input side is the per-word table xgate8).  ABI 9: the round-1 split step
     * (jlm_lstm_step_split: wt_split / kpad_split / xgate) is gone */
    float gate_descale, h_scale;
    const void *wt8; const float *xgate8;
    /* untied model on split rows (ABI 4; untied_split != NULL): the vocabulary matrix UM^T [V, H] as split rows scaled by
     * 2^eB, untied_descale = 2^-(14 + eB); the state rows plan.h are split rows then, plan.T their plain f32 copy */
    const void *untied_split; float untied_descale;
    /* ABI 9: 1 = the full-vocabulary normaliser on mixed rows runs jlm_vocab_lse_mixed_fr (no running maximum): set by the loader when
     * the model's own log-normalisers (load-time probe) sit well inside the f32 range */
    int lse_fixed_ref;
    /* T projection: [n_t, H] panel, plain or split rows */
    const float *pmt; const void *pmt_split; int n_t; float t_descale;
    /* full-vocabulary normaliser: split segments (NULL: f32 rows-stationary form) */
    const jlm_segment *split_segs; const float *split_t_scale; const float *split_descale; const int *split_bias_col;
    /* ABI 7: segments of that normaliser on MIXED rows (jlm_vocab_lse_hybrid; NULL: none): n_segs entries, mixed_segs[i].B ==
     * NULL leaves segment i on its split rows; mixed_t_scale / mixed_descale / mixed_s8 [n_segs] as for jlm_pack_t_mixed /
     * jlm_vocab_lse_mixed.  Used when the plan carries the packed-row buffer (plan.Tm). */
    const jlm_segment *mixed_segs; const float *mixed_t_scale; const float *mixed_descale; const float *mixed_s8;
    const float *mixed_bias2;       /* b2 log2(e) [V] for mixed segments without bias columns (NULL: none) */
    /* ABI 10: [n_segs] or NULL -- the leading words of a mixed segment that stay on split rows (jlm_vocab_lse_hybrid head_split) */
    const int *mixed_head_split;
} jlm_decode_model;

struct jlm_decode_cache;
struct jlm_decode_ngram;
struct jlm_decode_memory;
typedef struct {
    int kind;                       /* 0 static, full vocabulary; 1 static, selected vocabulary; 2 incremental */
    int max_cands;
    void *h; float *c; float *T;    /* [G, H] state rows (f32 or split), [G, H] f32, [G, ldt] f32 */
    const int *g0, *cidx, *sidx;    /* [n_frames*n_sent]: first row of a cell, cell index, sentence index */
    const int *sg_word, *sg_off, *sg_node;   /* lattice edges grouped by START (frame, sentence): word, CSR, node id */
    float *edge;                    /* == jlm_beam_state.edge */
    const int *vs_words, *vs_off; int vs_max;   /* kind 1: per-sentence selected vocabulary, longest list */
    /* kind 2: the vocabulary a (frame, sentence) cell c starts with = di_words[di_off[2c] .. di_off[2c+1])
     * (slices of per-sentence sequences, include/jlm_host.h jlm_dynamic_vocab); di_idx[c] = 2 * sentence */
    const int *di_words, *di_off, *di_idx; int di_max;
    const int *dd_words, *dd_off; int dd_max;   /* kind 2: words new at a frame, per (frame, sentence) */
    float *run_max; double *run_sum;            /* kinds 1, 2: running (max, sum exp) per row */
    float *part; int max_parts;                 /* kind 0: [max_parts][rmax][2] partial slices */
    /* kind 0: share (percent, 0 = all) of the CUs the vocabulary kernel may fill.  With two batches in flight on two streams
     * the other batch's latency-bound kernels (beam step, LSTM step, T projection) run on the CUs it leaves free instead of
     * behind it: 2.61 -> 2.33 ms per step at BASELINE configs[1] with 16 instead of 24 vocabulary ranges (tools/ab_np.py) */
    int lse_cu_share_pct;
    int *out_nodes; int *out_len; double *out_score; int stride;    /* jlm_backtrace outputs */
    /* kind 2 with a SEGMENTED projection, reference-compatibility mode (both NULL otherwise).  The reference's project()
     * returns a vocabulary subset's columns segment-major while DynamicDecoder indexes them -- and adds the bias -- in list
     * order (decoder_dynamic.py:76,130,172 over model.py:152-158,168-179), so list position j of a cell's first
     * vocabulary pairs the weight row of word di_wwords[j] with the bias and the identity of word di_words[j]; sg_wword[e]
     * is the word whose weight row the reference reads for lattice edge e (parallel to sg_word). */
    const int *di_wwords, *sg_wword;
    /* ABI 7, kind 0 with model.mixed_segs: [n_sent * beam][ld_tm] packed hypothesis rows of the frame being stepped
     * (jlm_pack_t_mixed over the model's mixed segments, right behind the T projection; ld_tm = jlm_mixed_t_stride of those) */
    void *Tm; int ld_tm;
    /* Left context (additive, ABI 12; both NULL: every sentence starts at <eos> from the zero state).  [n_sent * beam] device ints that
     * jlm_seed_context wrote: frame 0's LSTM step reads prev / word of sentence s's root row (g = s * beam) from them instead of
     * from jlm_beam_state.bp / .word -- it continues state row ctx_prev[g] (a row past the pool's n_frames * n_sent * beam rows, or
     * -1) and consumes ctx_word[g].  bp of frame 0 stays -1: jlm_backtrace stops at the root as before.  h / c then hold n_sent
     * more rows behind the pool. */
    const int *ctx_prev, *ctx_word;
    /* The continuous cache inside the frame loop (additive, ABI 12; NULL: the loop is what it was, launch for launch).  Kind 0 only:
     * see jlm_decode_cache below. */
    const struct jlm_decode_cache *cache;
    /* A back-off n-gram model mixed into every edge cost (additive, ABI 12; NULL: the loop is what it was, launch for launch).  Kind 0
     * only, and not together with `cache` (-1): see jlm_decode_ngram below. */
    const struct jlm_decode_ngram *ngram;
    /* A memory of (hidden state, next word) pairs mixed into every edge cost (additive, ABI 12; NULL: the loop is what it was, launch for
     * launch).  Kind 0 only, and not together with `cache` or `ngram` (-1): see jlm_decode_memory below. */
    const struct jlm_decode_memory *memory;
} jlm_decode_plan;

/* Returns 0 or a hipError_t.  st_host->lse_part / n_parts are managed by the call.  A full-vocabulary
 * model with a segment of k > 256 (untied: k = H, model.py:189-191) takes the tile form of the normaliser
 * (jlm_vocab_lse_partials per segment, one slice per 128 words: plan.max_parts >= the number of such tiles).
 *
 * events (may be NULL): JLM_EVENTS_PER_FRAME * n_frames hipEvent_t created by the caller (timing enabled).
 * They are recorded on `stream` around the kernel groups of every frame -- the edge logits then run on
 * `stream` too, so each bracket holds exactly what it names:
 *   [0] frame start  [1] after the incremental merge ("vocab fix", decoder_dynamic.py:112-148)
 *   [2] after the beam step ([1]..[2] = "lattice path fix" for the incremental decoder, :150-175)
 *   [3] after the LSTM step ([2]..[3] = perf_log_lstm, decoder.py:206-218; the gate GEMM alone)
 *   [4] after the T projection and the edge logits   [5] after the normaliser ([4]..[5] = the vocabulary
 *   kernel alone; [3]..[5] = perf_log_softmax).  Frames past the last stepped one record [0]..[2] only. */
#define JLM_EVENTS_PER_FRAME 6
int jlm_decode_frames(const jlm_decode_model *model_host, const jlm_decode_plan *plan_host,
                      const jlm_lattice *lat_host, const jlm_beam_state *st_host,
                      void *stream, void *side_stream, void *const *events);

/* ABI 8: probe of the full-vocabulary normaliser, for the load-time calibration of the mixed rows (jlm_amd/model.py
 * DeviceModel._calibrate_mixed; the reference computes every logit in float64, decoder/model.py:141-193,15-20 -- which
 * int8 cross terms can follow only as far as the model's logit range lets them).  Runs `steps` LSTM steps (jlm_lstm_step_xg)
 * of `rows` hypotheses from the zero state -- row g = t * rows + r is hypothesis r after t steps: rowlist[g] = g,
 * prev[g] = g - rows (negative in block 1), word[g] = the word step t consumes; h, c [(steps + 1) * rows, H], T
 * [(steps + 1) * rows, ldt] -- then the T projection of the last block and its normaliser slices into part [max_parts][rows][2]:
 * form 0 = jlm_vocab_lse_split, form 1 = what jlm_decode_frames launches with the model's mixed rows (jlm_pack_t_mixed into
 * Tm [rows][ld_tm] + jlm_vocab_lse_mixed / jlm_vocab_lse_hybrid).  Returns the number of slices (>= 1), -2 for a model
 * without that form, -1 / a hipError_t as the launchers do. */
int jlm_lse_probe(const jlm_decode_model *model_host, const int *rowlist, const int *prev, const int *word, int steps, int rows,
                  void *h, float *c, float *T, void *Tm, int ld_tm, int form, float *part, int max_parts, void *stream);


/* ------------------------------------------------------------------------
 * Teacher-forced scoring (LSTM_Model.score / score_streams, jlm_amd/score.py): the per-word -log p of many word sequences at
 * once -- what the reference's LSTM_Model.evaluate (decoder/model.py:200-206) computes one predict() at a time, and what its
 * training script reports as test perplexity (train/model.py:262-297 over train/utils.py:17-31 corpus_iterator).
 * Row r < n_rows is one sequence (or one stream).  Step t consumes word[t][r] and is scored on target[t][r]:
 *   nll = lse(T_r) - (T_r[t_off:t_off+k] . B_seg[w - v_start] + b2[w]),  w = target[t][r]   (self_norm models: nll = -y)
 * The rows live at step t are the prefix r < n_live[t] (the caller sorts sequences by length, longest first).
 * State: two row sets h[2] / c[2] ([n_rows, H] each; split rows on a split-row model, plain f32 otherwise, as jlm_decode_plan.h /
 * .c), used ping-pong -- step t reads set t % 2 and writes set (t + 1) % 2 (never in place: several workgroups of the step read a
 * row another one writes).  Step 0 continues row prev0[r] of set 0 (-1: the zero state); the state after the last step is in set
 * n_steps % 2. */
typedef struct {
    int n_rows, n_steps;
    void *h[2]; float *c[2];        /* [n_rows, H] state row sets */
    float *T;                       /* [n_rows, ldt] f32 (untied split-row model: the state's f32 copy; untied f32 model: unused) */
    void *Tm; int ld_tm;            /* packed rows for a normaliser on mixed rows (as jlm_decode_plan.Tm), or NULL */
    float *part; int max_parts;     /* [max_parts][n_rows][2] normaliser slices (as jlm_decode_plan.part) */
    const int *rows;                /* [n_rows] device: 0, 1, ..., n_rows - 1 (the compact row list; also the prev of steps t >= 1) */
    const int *prev0;               /* [n_rows] device: the row of set 0 that step 0 continues, -1 = zero state */
    const int *word, *target;       /* [n_steps][n_rows] device */
    const int *n_live;              /* [n_steps] device */
    const int *n_live_host;         /* [n_steps] host copy (bounds the launches' grids), or NULL: n_rows */
    double *nll_seq;                /* [n_rows] device: += the row's nll of every step (the caller zeroes it) */
    double *nll_tok;                /* [n_steps][n_rows] device, or NULL: the nll of each (step, live row) */
    int *flags;                     /* one device int or NULL: |= 1 when a log-normaliser is not finite (as jlm_beam_state.flags) */
} jlm_score_plan;

/* Enqueues n_steps x [LSTM step (jlm_lstm_step_xg | jlm_lstm_step), T projection (not on untied models), the full-vocabulary
 * normaliser exactly as jlm_decode_frames launches it for kind 0 (none on self_norm models), score_fold_kernel (the slices folded
 * in the beam step's order and arithmetic, the target's logit in jlm_edge_logits' f32 arithmetic, nll in f64)].  No host
 * synchronisation.  events (may be NULL): JLM_SCORE_EVENTS_PER_STEP * n_steps hipEvent_t (timing enabled), recorded on `stream`
 *   [0] before the LSTM step  [1] after it  [2] after the T projection  [3] after the normaliser  [4] after the fold.
 * Returns 0, -2 for a model outside the frame loop's shapes, -1 / a hipError_t as the launchers do. */
#define JLM_SCORE_EVENTS_PER_STEP 5
int jlm_score_frames(const jlm_decode_model *model_host, const jlm_score_plan *plan_host, void *stream, void *const *events);

/* ABI 12 (additive): the last launch of a scoring step on its own (csrc/jlm_score.hip, score_fold_kernel; jlm_score_frames calls it
 * once per step with the step's rows of target / nll_tok).  For every row r < min(*n_dev, n_rows_max) (n_dev NULL: n_rows_max), with
 * w = target[r] and the segment sg that holds w:
 *   lse = log sum_p part[p][r].sum * exp(part[p][r].max) over the n_parts slices part[(p * ld_part + r) * 2 + {0: max, 1: sum exp}]
 *         (f32 maxima and exponentials, f64 sums; not read and taken as 0 for self_norm != 0)
 *   y   = T[r * ldt + sg.t_off .. + sg.k) . sg.B[(w - sg.v_start) * sg.ldb .. + sg.k) + b2[w]     (f32, fmaf)
 *   nll = lse - y (f64);  nll_seq[r] += nll;  nll_tok[r] = nll when nll_tok != NULL.
 * flags (one device int, may be NULL): |= 1 when a row's lse is not finite (its nll is stored as computed), |= 2 when a row's target
 * lies in no segment -- that row's nll is NaN, nothing of B, T or b2 is read for it.  Rows from min(*n_dev, n_rows_max) on are left
 * alone in nll_seq and nll_tok.  -1: n_segs out of range, or ldt / a segment's k, ldb or t_off not a multiple of 4. */
int jlm_score_fold(const jlm_segment *segs_host, int n_segs, const float *b2, const float *T, int ldt, const float *part, int ld_part,
                   int n_parts, int self_norm, const int *target, const int *n_dev, int n_rows_max, double *nll_seq, double *nll_tok,
                   int *flags, void *stream);

/* ------------------------------------------------------------------------
 * Ancestral sampling (LSTM_Model.generate, jlm_amd/generate.py): what the reference's sample(pred, temperature) and its sampling
 * loop do one predict() at a time on the host (decoder/model.py:28-33, 213-245; train/test.py).
 *
 * jlm_sample_rows: one draw per row r < min(n_rows_max, *n_dev) (n_dev may be NULL) of f32 logits y[r * ld_y + 0 .. n_cols) in word-id
 * order (ld_y % 4 == 0, ld_y >= n_cols rounded up to 4, y 16-byte aligned).  With m = max y, tau = temperature, inv = (float)(1 / tau):
 *   S = sum_j expf((y_j - m) * inv)  (f32 exp, f64 sums; the order is a fixed function of n_cols and the launch)
 *   u = uniform(seed, step, row_id[r] (NULL: r)):  z = seed + 0x9E3779B97F4A7C15 * ((step << 32) | (row + 1)) (uint64, wrapping),
 *       z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9, z = (z ^ (z >> 27)) * 0x94D049BB133111EB, z ^= z >> 31, u = ((z >> 11) + 0.5) 2^-53
 *   draw = the smallest i with sum_{j <= i} expf((y_j - m) * inv) > u S; if rounding leaves no crossing, the last word with mass.
 *   temperature 0: the argmax, the lowest id winning a tie.
 * Per row: ids[r] = word[r] = the draw, nll[r] = -log p at tau = 1 in f64 (lse - y; self_norm: -y).  forced (or NULL): forced[r] >= 0
 * passes through (word[r] = forced[r], ids[r] = -1, nll[r] = 0).  done (or NULL): a row with done[r] != 0 is masked (ids -1, nll 0,
 * word unchanged); a draw equal to stop_id sets done[r] = 1.  A non-finite max or sum: *flags |= 1, ids -1, nll NaN, word 0.
 * Returns 0, -1 for arguments the kernel cannot handle (temperature < 0 or not finite included), or a hipError_t. */
int jlm_sample_rows(const float *y, int ld_y, int n_cols, int n_rows_max, const int *n_dev, double temperature, uint64_t seed, int step,
                    const int *row_id, const int *forced, int *done, int stop_id, int self_norm, int *word, int *ids, double *nll,
                    int *flags, void *stream);

/* jlm_sample_rows_trunc: jlm_sample_rows' draw over a truncated distribution; every argument it shares with jlm_sample_rows means
 * what it means there.  Words are ranked by (y_j descending, id ascending): a rank order of the logits, so it does not depend on
 * the temperature.  With the masses w_j = expf((y_j - m) * inv) of jlm_sample_rows:
 *   top_k   the kept set K is the first min(top_k, n_cols) words in rank order; top_k <= 0 or >= n_cols: off (K is every word).
 *   top_p   (0 < top_p; >= 1: off) within K, the shortest prefix in rank order whose mass is >= top_p * mass(K); at least one word.
 *           Top-k first, then top-p on what it kept.  The cut compares exact fixed-point sums of the f32 masses (each rounded to a
 *           multiple of 2^-s, s = min(52, 62 - ceil(log2 n_cols))), so it does not depend on the order of summation.
 *   draw    jlm_sample_rows' inverse CDF in word-id order over the kept words only, with the same u: the smallest kept i with
 *           sum_{kept j <= i} w_j > u S_kept; if rounding leaves no crossing, the last kept word with mass.
 *   temperature 0: greedy as jlm_sample_rows, whatever top_k and top_p are; top_k = 1 is the same argmax (lowest id on a tie).
 * nll[r] is unchanged: the draw's -log p under the FULL distribution at tau = 1 (lse - y; self_norm: -y), comparable with
 * jlm_score_frames.  forced, done / stop_id, n_dev and flags behave as in jlm_sample_rows (a NaN anywhere in a row flags it).  With
 * both off, or temperature 0, this IS jlm_sample_rows (the same kernel).  The selection reads a row a bounded number of times
 * (at most 9.75 with the draw, whatever top_k, top_p and n_cols are) and the result is bit-identical run to run.
 * Returns 0, -1 for arguments the kernel cannot handle (top_p <= 0 or NaN included), or a hipError_t. */
int jlm_sample_rows_trunc(const float *y, int ld_y, int n_cols, int n_rows_max, const int *n_dev, double temperature, uint64_t seed,
                          int step, const int *row_id, const int *forced, int *done, int stop_id, int self_norm, int top_k, double top_p,
                          int *word, int *ids, double *nll, int *flags, void *stream);

/* The sampling loop.  Row r < n_rows is one prompt; prompts are RIGHT-aligned on n_prompt frames (the caller sorts rows by prompt
 * length, longest first, so the rows live at prompt frame f are the prefix r < n_live[f]; every row is live at frame n_prompt - 1).
 * Frame f < n_prompt consumes prompt[f][r] and continues row prev[f][r] (-1: the zero state, at a row's first frame); frame
 * f >= n_prompt consumes word[r] (what the previous frame drew) and continues row r.  Frames n_prompt - 1 .. n_prompt + n_words - 2
 * draw: draw k = frame - (n_prompt - 1) goes to ids[k][r], nll[k][r] (sample_rows_kernel with step = k, row_id).  State: h[2] / c[2]
 * ping-pong as jlm_score_plan's. */
typedef struct {
    int n_rows, n_prompt, n_words;
    void *h[2]; float *c[2];        /* [n_rows, H] state row sets (both zeroed or not: rows start from prev = -1) */
    float *T;                       /* [n_rows, ldt] f32 (as jlm_score_plan.T) */
    float *logits; int ld_logits;   /* [n_rows, ld_logits] f32, ld_logits >= V rounded up to 4 */
    const int *rows;                /* [n_rows] device: 0, 1, ..., n_rows - 1 */
    const int *prev, *prompt;       /* [n_prompt][n_rows] device */
    const int *n_live;              /* [n_prompt] device */
    const int *n_live_host;         /* [n_prompt] host */
    const int *row_id;              /* [n_rows] device: the row's index in the caller's list (the random numbers' row), or NULL: r */
    int *word;                      /* [n_rows] device: the word the next frame consumes */
    int *done;                      /* [n_rows] device, zeroed, or NULL (no stop word) */
    int stop_id;
    double temperature;             /* >= 0; 0 = greedy */
    uint64_t seed;
    int *ids; double *nll;          /* [n_words][n_rows] device */
    int *flags;                     /* one device int or NULL */
} jlm_generate_plan;

/* Enqueues n_prompt + n_words - 1 frames of [LSTM step (the launches jlm_score_frames makes), and on drawing frames the T projection,
 * jlm_gemm_nt per segment into plan.logits (+ b2), sample_rows_kernel].  No host synchronisation.  events (may be NULL):
 * JLM_GENERATE_EVENTS_PER_FRAME * frames hipEvent_t, recorded on `stream` [0] before the LSTM step [1] after it [2] after the T
 * projection [3] after the logit GEMMs [4] after the draw (prompt frames: empty brackets after [1]).  Returns 0, -2 for a model
 * outside the loop's shapes, -1 / a hipError_t as the launchers do. */
#define JLM_GENERATE_EVENTS_PER_FRAME 5
int jlm_generate_frames(const jlm_decode_model *model_host, const jlm_generate_plan *plan_host, void *stream, void *const *events);

/* jlm_generate_frames with every draw made by jlm_sample_rows_trunc(..., top_k, top_p, ...): the same loop, plan and event brackets. */
int jlm_generate_frames_trunc(const jlm_decode_model *model_host, const jlm_generate_plan *plan_host, int top_k, double top_p,
                              void *stream, void *const *events);

/* ------------------------------------------------------------------------
 * Next-word prediction and beam-search completion (LSTM_Model.predict_top / complete, jlm_amd/complete.py): the reference's
 * find_top_N (decoder/model.py:25-26, an argsort of one host-side distribution) for many rows, and an n-best continuation loop.
 *
 * jlm_topk_rows: per row r < n_rows of f32 logits y[r * ld_y + 0 .. n_cols) (ld_y % 4 == 0, ld_y >= n_cols rounded up to 4, y 16-byte
 * aligned; the row is read once), its k best words ranked by y descending, equal logits lower id first (the greedy draw's rule):
 * ids[r * ld_out + i], i < k, and nll[r * ld_out + i] = lse - y in f64 with lse = m + log S, m = max y, S = sum_j expf(y_j - m_j)
 * rescaled in f64 to m (f32 exp, f64 sums, a fixed order for a given n_cols; within ~1e-7 of the f64 lse); self_norm: nll = -y.
 * A non-finite max or sum: *flags |= 1 (flags may be NULL), the row's ids -1 and nll NaN.  1 <= k <= min(JLM_TOPK_MAX, n_cols),
 * ld_out >= k.  Returns 0, -1 for arguments the kernel cannot handle, or a hipError_t. */
#define JLM_TOPK_MAX 64
int jlm_topk_rows(const float *y, int ld_y, int n_cols, int n_rows, int k, int self_norm, int *ids, double *nll, int ld_out, int *flags,
                  void *stream);

/* jlm_topk_rows with each row's candidates restricted to a word set.  mask: [n_sets][ld_mask] 32-bit words on the device, bit w & 31 of
 * word w >> 5 of set s says that word w is allowed (ld_mask >= ceil(n_cols / 32)); row_set: [n_rows] device ints, the set of row r, or
 * -1 for an unrestricted row, which loads no mask and gives jlm_topk_rows' output bit for bit.  The log-normaliser is jlm_topk_rows':
 * it runs over every word of the row, in the same order and arithmetic, so nll stays -log p under the full distribution and a
 * disallowed word may hold the row's maximum.  Only allowed words are ranked (y descending, id ascending; NaN never ranks, -inf
 * does).  A restricted row with m < k rankable words returns those m, then ids -1 and nll +inf at m .. k - 1: no error, no flag.  A
 * non-finite max or sum flags the row as jlm_topk_rows does (ids -1, nll NaN), whether or not the offending word is allowed; so does a
 * row_set[r] outside [-1, n_sets), which indexes nothing (torch.ops.jlm.topk_rows_masked refuses it on the host).  Argument checks as
 * jlm_topk_rows, and n_sets >= 0, row_set != NULL, with n_sets > 0 mask != NULL and ld_mask as above.  n_sets = 0 needs no mask. */
int jlm_topk_rows_masked(const float *y, int ld_y, int n_cols, int n_rows, int k, int self_norm, const unsigned *mask, int ld_mask,
                         int n_sets, const int *row_set, int *ids, double *nll, int ld_out, int *flags, void *stream);

/* jlm_beam_merge: one beam-search selection per prompt p < n_prompts over per-row top-`beam` lists (jlm_topk_rows with k = ld_out =
 * beam).  first != 0: the prompt's one candidate row is p, its score 0; else rows p * beam + j, j < beam (rank j of the previous beam)
 * with score[row] and finished[row].  A candidate is (score + nll, parent rank j, word); a finished parent gives one carry (its score,
 * word -1) instead of its row's list.  The beam best by (score ascending, parent rank ascending, word ascending) -- per row taken in
 * list order, equal f64 scores lower word first -- go to rows q = p * beam + i, i = rank: score[q], finished[q] (a carry, or a word
 * equal to stop_id when stop_id >= 0), word[q] (the word the next LSTM step consumes: the word, or for a carry max(stop_id, 0)),
 * prev[q] (the parent's row: first ? p : p * beam + j), and the back-pointers bp_parent[q] = j, bp_word[q] (-1: carry),
 * bp_nll[q] (0: carry).  score / finished are read and written in place.  Returns 0, -1 for bad arguments, or a hipError_t. */
int jlm_beam_merge(const int *cand_ids, const double *cand_nll, int beam, int n_prompts, int first, int stop_id, int *word, int *prev,
                   double *score, int *finished, int *bp_parent, int *bp_word, double *bp_nll, void *stream);

/* The beam-search loop.  n_prompts prompts, RIGHT-aligned on n_prompt frames and sorted longest first, as jlm_generate_plan's rows:
 * prompt frames step the live prefix r < n_live[f] of rows 0 .. n_prompts - 1, consuming prompt[f][r] and continuing prev[f][r].
 * The last prompt frame (f = n_prompt - 1) is selecting frame 0: the T projection, the logits and jlm_topk_rows over those n_prompts
 * rows, then jlm_beam_merge (first = 1).  Each later frame f (selecting frame k = f - n_prompt + 1, up to n_words - 1) steps all
 * R = n_prompts * beam rows, consuming word[r] and continuing row prev_row[r] of the set being read (what the previous merge wrote),
 * then the T projection, the logits, jlm_topk_rows and jlm_beam_merge (first = 0).  Back-pointers of frame k at bp_*[k * R + q].
 * After the call score[q] / finished[q] hold the final beam, rank i of prompt p at q = p * beam + i.  State h[2] / c[2] ping-pong as
 * jlm_generate_plan's. */
typedef struct {
    int n_prompts, beam, n_prompt, n_words;
    void *h[2]; float *c[2];        /* [R, H] state row sets, R = n_prompts * beam */
    float *T;                       /* [R, ldt] f32 (as jlm_generate_plan.T) */
    float *logits; int ld_logits;   /* [R, ld_logits] f32, ld_logits >= V rounded up to 4 */
    const int *rows;                /* [R] device: 0, 1, ..., R - 1 */
    const int *prev, *prompt;       /* [n_prompt][n_prompts] device */
    const int *n_live;              /* [n_prompt] device */
    const int *n_live_host;         /* [n_prompt] host */
    int *cand_ids; double *cand_nll;    /* [R][beam] device: the per-row lists */
    int *word, *prev_row;           /* [R] device: the next frame's inputs (the merge writes them) */
    double *score; int *finished;   /* [R] device */
    int stop_id;                    /* < 0: none */
    int *bp_parent, *bp_word;       /* [n_words][R] device */
    double *bp_nll;                 /* [n_words][R] device */
    int *flags;                     /* one device int or NULL */
} jlm_complete_plan;

/* Enqueues n_prompt + n_words - 1 frames of [LSTM step (the launches jlm_generate_frames makes), and on selecting frames the T
 * projection, jlm_gemm_nt per segment into plan.logits (+ b2), jlm_topk_rows, jlm_beam_merge].  No host synchronisation.  events (may
 * be NULL): JLM_COMPLETE_EVENTS_PER_FRAME * frames hipEvent_t, recorded on `stream` [0] before the LSTM step [1] after it [2] after the
 * T projection [3] after the logit GEMMs [4] after the selection [5] after the merge (prompt frames: empty brackets after [1]).
 * 1 <= beam <= min(JLM_TOPK_MAX, V).  Returns 0, -2 for a model outside the loop's shapes, -1 / a hipError_t as the launchers do. */
#define JLM_COMPLETE_EVENTS_PER_FRAME 6
int jlm_complete_frames(const jlm_decode_model *model_host, const jlm_complete_plan *plan_host, void *stream, void *const *events);

/* jlm_complete_frames with the first generated word of prompt p restricted to set prompt_set[p] (device ints [n_prompts], -1:
 * unrestricted) of mask [n_sets][ld_mask] (device, as jlm_topk_rows_masked's): selecting frame 0 selects with jlm_topk_rows_masked,
 * every later frame is jlm_complete_frames'.  The same loop, plan and event brackets.  A set with fewer than `beam` rankable words
 * leaves frame 0's list padded with (-1, +inf); jlm_beam_merge turns a padded candidate into a finished hypothesis of score +inf (word
 * -1), which is carried, never expanded, ranks behind every finite candidate and leaves the beam as soon as the live hypotheses offer
 * `beam` candidates: the caller drops final hypotheses whose score is not finite. */
int jlm_complete_frames_masked(const jlm_decode_model *model_host, const jlm_complete_plan *plan_host, const unsigned *mask, int ld_mask,
                               int n_sets, const int *prompt_set, void *stream, void *const *events);

/* ------------------------------------------------------------------------
 * The rank of the word that was actually written (LSTM_Model.rank / rank_streams, jlm_amd/rank.py): top-k accuracy, mean
 * reciprocal rank, keystroke savings and the position among homophones all follow from it.  Additive to ABI 12.
 *
 * jlm_rank_rows: for every row r < min(*n_dev, n_rows_max) (n_dev NULL: n_rows_max) of f32 logits y[r * ld_y + 0 .. n_cols) (ld_y %
 * 4 == 0, ld_y >= n_cols rounded up to 4, y 16-byte aligned) with t = target[r], and for a set S of word ids, the 0-based
 *   rank(S) = #{ w in S : y[w] > y[t] } + #{ w in S : w < t and y[w] == y[t] }
 * -- jlm_topk_rows' order (logit descending, lower id first on a tie), IEEE comparisons: a NaN y[w] is never counted, +-inf compare
 * as they do.  The normaliser does not enter, so self-normalised and ordinary models rank alike.
 * rank [n_rows][n_levels + 1] int32:
 *   column 0       S = every word 0 .. n_cols - 1 (level A)
 *   column 1 + i   S = { ids[j] : lv_lo[e] <= j < lv_hi[e] }, e = lv_off[t] + i, for i < min(lv_off[t + 1] - lv_off[t], n_levels): entry
 *                  i of the target's level list, a CSR table over the words (lv_off [n_cols + 1]; spans are cut to [0, n_ids), an id
 *                  outside [0, n_cols) is no word and nothing is read for it).  ids [n_ids] is ReadingIndex's order, (reading, id).
 *   every column the target has no entry for holds -1.  lv_off NULL: level A only (ids / lv_lo / lv_hi are not read).
 * A NaN y[t]: -1 in every column of the row, *flags |= 1.  A target outside [0, n_cols): -1 in every column, *flags |= 2, nothing is
 * indexed by it.  flags: one device int, may be NULL.  Rows from min(*n_dev, n_rows_max) on are not touched.  The counts are
 * integers: the result is the same bits run to run and whatever the launch shape.
 * Returns 0, -1 for arguments the kernel cannot handle (jlm_topk_rows' conditions on y; n_levels outside 0 .. JLM_RANK_MAX_LEVELS;
 * target or rank NULL; lv_off without lv_lo / lv_hi, or without ids when n_ids > 0), or a hipError_t. */
#define JLM_RANK_MAX_LEVELS 32
int jlm_rank_rows(const float *y, int ld_y, int n_cols, int n_rows_max, const int *n_dev, const int *target, const int *ids, int n_ids,
                  const int *lv_off, const int *lv_lo, const int *lv_hi, int n_levels, int *rank, int *flags, void *stream);

/* The ranking loop: jlm_score_plan's rows, steps, n_live and prev0 (row r is one sequence or stream, step t consumes word[t][r],
 * the rows live at step t are the prefix r < n_live[t], state sets ping-pong, step 0 continues row prev0[r] of set 0) with the
 * materialised logits of jlm_generate_plan and the level table of jlm_rank_rows. */
typedef struct {
    int n_rows, n_steps;
    void *h[2]; float *c[2];        /* [n_rows, H] state row sets */
    float *T;                       /* [n_rows, ldt] f32 (as jlm_score_plan.T) */
    float *logits; int ld_logits;   /* [n_rows, ld_logits] f32, ld_logits >= V rounded up to 4 */
    const int *rows;                /* [n_rows] device: 0, 1, ..., n_rows - 1 */
    const int *prev0;               /* [n_rows] device: the row of set 0 that step 0 continues, -1 = zero state */
    const int *word, *target;       /* [n_steps][n_rows] device */
    const int *n_live;              /* [n_steps] device */
    const int *n_live_host;         /* [n_steps] host copy (bounds the launches' grids), or NULL: n_rows */
    const int *ids; int n_ids;      /* the level table of jlm_rank_rows (lv_off NULL: level A only) */
    const int *lv_off, *lv_lo, *lv_hi;
    int n_levels;
    int *rank;                      /* [n_steps][n_rows][n_levels + 1] device: the live rows of every step are written */
    int *flags;                     /* one device int or NULL: jlm_rank_rows' bits */
} jlm_rank_plan;

/* Enqueues n_steps x [LSTM step and T projection of the live rows (the launches jlm_score_frames makes), jlm_gemm_nt per segment into
 * plan.logits (+ b2) as jlm_generate_frames makes them on a drawing frame, rank_rows_kernel on target[t]].  No host synchronisation.
 * events (may be NULL): JLM_RANK_EVENTS_PER_STEP * n_steps hipEvent_t (timing enabled), recorded on `stream`
 *   [0] before the LSTM step  [1] after it  [2] after the T projection  [3] after the logit GEMMs  [4] after the ranking.
 * Returns 0, -2 for a model outside the loop's shapes, -1 / a hipError_t as the launchers do. */
#define JLM_RANK_EVENTS_PER_STEP 5
int jlm_rank_frames(const jlm_decode_model *model_host, const jlm_rank_plan *plan_host, void *stream, void *const *events);

/* ------------------------------------------------------------------------
 * The continuous cache of teacher-forced scoring (LSTM_Model.score_cached / score_streams_cached, jlm_amd/cache.py; Grave, Joulin,
 * Usunier, "Improving neural language models with a continuous cache", ICLR 2017).  Additive to ABI 12.
 *
 * Take one row, a sequence or a stream.  Position j is the step that consumes word[j]; it leaves the hidden state h_j and is scored
 * on w_j = target[j].  Positions are numbered over the whole life of a stream, across calls.  The cache before position q holds the
 * pairs (h_i, w_i) for max(q - N, first) <= i < q, first = the row's oldest existing position; n_q is their count.
 *   s_i       = theta * (h_q . h_i)                       h in real units (split rows: (hi + lo) / h_scale)
 *   lpc_q     = log sum_{i : w_i = w_q} exp(s_i) - log sum_i exp(s_i)       (-inf when no i matches, and when n_q = 0: unused there)
 *   p_q       = (1 - lambda) exp(-nll_q) + lambda exp(lpc_q)   when n_q > 0;   exp(-nll_q) when n_q = 0
 *   nll_mix_q = -log p_q                                   (float64, on the host, via logaddexp: jlm_amd/cache.py)
 * nll_q is what score_fold_kernel writes (self_norm models: -y).  Word ids are only ever compared, never used as an index.
 * Ranges: N >= 1, theta >= 0, 0 <= lambda < 1.
 *
 * jlm_cache_rows (csrc/jlm_cache.hip, cache_rows_kernel): lpc of n_query consecutive positions pos0 .. pos0 + n_query - 1 of n_rows
 * rows, for n_theta values of theta, from two rings:
 *   hist  [cap][n_rows][H]   state rows in the model's state-row format, 4 bytes a value either way: split != 0 the split rows the
 *                            LSTM step writes ([8 hi][8 lo] f16 of h * h_scale), else plain f32 (h_scale is not read); 16-byte aligned
 *   words [cap][n_rows]      int32: w_i
 * The slot of logical position j is j mod cap; the queries' own states and words are in the rings (cap >= N + n_query, so that no
 * query's slot is an entry of another's window).  first [n_rows] device: row r's oldest existing position (>= 0); len [n_rows]
 * device: the number of queries of row r, the positions pos0 .. pos0 + len[r] - 1 (rows are sorted longest first, so a row's queries are
 * a prefix of the steps); thetas [n_theta] HOST floats, 1 <= n_theta <= JLM_CACHE_MAX_THETAS.
 *   lpc [n_theta][n_query][n_rows] f32; entries (q, r) with q >= len[r] are left untouched.
 *   flags (one device int, may be NULL): |= 1 when the product h_q . h_i of an entry inside a query's window is not finite.  A slot
 *   outside every window is never read.
 * Arithmetic: the products h_q . h_i come off the matrix pipe -- split rows: hi.hi + hi.lo + lo.hi in three v_mfma_f32_32x32x16_f16
 * per 16 k with f32 accumulation over the stored halves, 1 / h_scale^2 folded into theta; f32 rows: v_mfma_f32_32x32x2_f32, an f32 fmaf
 * chain over k -- s = f32(theta' * dot); the two sums are f32 online sums under one running maximum, expf / logf the f32 library
 * functions, lpc = logf(M) - logf(Z).  The values of theta are independent of one another: lpc[t] is the same bits whatever else
 * thetas holds.  The order of the sums depends on pos0 and the window, so the same window reached by another cut of a stream may
 * differ within the rounding bound (tests/test_gpu_cache_rows.py derives it).
 * Returns -1 before any launch for cap < N + n_query, N < 1, H <= 0 or H % 32 != 0 (what jlm_lstm_step / jlm_lstm_step_xg accept),
 * hist not 16-byte or another pointer not 4-byte aligned or NULL, n_theta out of range, a theta that is negative or not finite,
 * pos0 < 0 or pos0 + n_query + cap >= 2^31, n_rows > 65535, split != 0 with h_scale <= 0; 0 with nothing launched for n_rows == 0
 * or n_query == 0; else 0 or a hipError_t. */
#define JLM_CACHE_MAX_THETAS 16
int jlm_cache_rows(const void *hist, const int *words, int cap, int n_rows, int H, int split, float h_scale, int pos0, int n_query,
                   const int *first, const int *len, int N, const float *thetas_host, int n_theta, float *lpc, int *flags, void *stream);

/* What a cached scoring call has beside its jlm_score_plan (whose layout is unchanged): the rings of jlm_cache_rows over the plan's
 * n_rows rows, step t of the plan being position pos0 + t. */
typedef struct {
    void *hist; int *words; int cap;    /* the rings; the entries carried into the call are in their slots already */
    int pos0;                           /* the position of step 0 */
    const int *first;                   /* [n_rows] device */
    const int *len;                     /* [n_rows] device: the steps row r is live */
    int N;
    const float *thetas; int n_theta;   /* host */
    float *lpc;                         /* [n_theta][n_steps][n_rows] device */
    int *flags;                         /* one device int or NULL: jlm_cache_rows' bit */
} jlm_cache_plan;

/* jlm_score_frames' loop -- the same launches in the same order, so nll_seq / nll_tok are the same bits -- with two additions: after
 * step t the live rows of the state set the step wrote are copied into hist[slot(pos0 + t)] (an asynchronous device-to-device copy on
 * `stream`, in the raw state-row format: one small launch) and the step's targets into words at the same slot; after the last step jlm_cache_rows runs
 * once over the n_steps query positions.  No host synchronisation.  Every refusal of jlm_cache_rows is returned before the first
 * launch.  events as jlm_score_frames'.  Returns as jlm_score_frames does. */
int jlm_score_cache_frames(const jlm_decode_model *model_host, const jlm_score_plan *plan_host, const jlm_cache_plan *cache_host,
                           void *stream, void *const *events);

/* ------------------------------------------------------------------------
 * Scoring against a memory of hidden states (LSTM_Model.score_memory / score_streams_memory, jlm_amd/memory.py, DESIGN.md section 28;
 * the unbounded cache of Grave, Cisse and Joulin, NIPS 2017 -- with exact search, the datastore of a kNN-LM).  Additive to ABI 12.
 *
 * A memory is N >= 1 entries (k_i, v_i): k_i a hidden state in the model's state-row format, v_i the id of the word that followed it.
 * It is built once, stays on the device and is shared by every row of every call.  A query position q has the state h_q and is scored
 * on w_q, exactly as a position of the cache above.  For every theta of the call
 *   s_i       = theta * (h_q . k_i)                       h, k in real units (split rows: (hi + lo) / h_scale)
 *   lpm_q     = log sum_{i : v_i = w_q} exp(s_i) - log sum_{i < N} exp(s_i)     (-inf when no i matches)
 *   p_q       = (1 - lambda) exp(-nll_q) + lambda exp(lpm_q)
 *   nll_mix_q = -log p_q                                   (float64, on the host: jlm_amd/cache.py mix_nll with n_entries = N)
 * There is no causality and no window: every query sees every entry.  Word ids are only ever compared, never used as an index.
 * Ranges: theta >= 0 and finite, 0 <= lambda < 1, 1 .. JLM_CACHE_MAX_THETAS values of theta a call, N <= JLM_MEMORY_MAX_KEYS.
 *
 * jlm_memory_rows (csrc/jlm_memory.hip: memory_rows_kernel, memory_fold_kernel):
 *   keys      [N][H]                 state rows, 4 bytes a value either way (split != 0: [8 hi][8 lo] f16 of k * h_scale; else f32, and
 *                                    h_scale is not read); 16-byte aligned.   key_words [N] int32
 *   q_rows    [n_steps][n_rows][H]   the queries' state rows in the same format, q_words [n_steps][n_rows] int32: what the store hook of
 *                                    jlm_score_cache_frames leaves in a ring with nothing carried.  Query (t, r) is live iff t < len[r]
 *                                    (len [n_rows] device int32; NULL: every query is live); rows and words of queries that are not
 *                                    live are never read.
 *   lpm       [n_theta][n_steps][n_rows] f32; entries of queries that are not live are left untouched.
 *   flags     (one device int, may be NULL): |= 1 when a product h_q . k_i of a live query is not finite.
 * The key split.  The keys are cut into ceil(N / S) consecutive ranges of S = jlm_memory_keys_per_split(N) keys, a function of N ALONE:
 *   S = max(JLM_MEMORY_MIN_SPLIT_KEYS, ceil(ceil(N / JLM_MEMORY_MAX_SPLITS) / 64) * 64)
 * -- 512 keys, one pair of 32-key tiles per wave, grown so that there are never more than 128 splits.  The grid is (block of 32
 * queries) x (split), query block fastest.  A workgroup folds its range under cache_rows_kernel's arithmetic and in its fixed order
 * (wave w: tile pairs w, w + 8, ...; the two half-waves; the eight waves) and writes one partial (m, Z, M) per (theta, split, query) to
 * the workspace, [n_theta][n_split][3][n_steps * n_rows] f32, jlm_memory_workspace_bytes(N, n_rows, n_steps, n_theta) bytes;
 * memory_fold_kernel folds a query's splits in ascending order and writes logf(M) - logf(Z).  Every word of the workspace that is read
 * was written by the same call.  Arithmetic of the products, scores and sums: jlm_cache_rows'.
 * The bits of lpm for (query state row, query word, theta, memory) do not depend on how many queries or thetas the call carries, on
 * which other queries are live, on where in the call the query stands, or on what the workspace held before.
 * Returns -1 before any launch for N < 1 or N > JLM_MEMORY_MAX_KEYS, H <= 0 or H % 32 != 0, n_theta out of range or thetas NULL, a
 * theta that is negative or not finite, split != 0 with h_scale <= 0, n_rows or n_steps < 0, n_rows > 65535,
 * n_rows * n_steps >= 2^27, keys / q_rows not 16-byte or another pointer not 4-byte aligned, a NULL pointer other than len and flags,
 * workspace_bytes below jlm_memory_workspace_bytes(...); 0 with nothing launched for n_rows == 0 or n_steps == 0 (after the checks on
 * N, H, thetas and h_scale); else 0 or a hipError_t. */
#define JLM_MEMORY_MAX_KEYS (1 << 24)
#define JLM_MEMORY_MIN_SPLIT_KEYS 512
#define JLM_MEMORY_MAX_SPLITS 128
int jlm_memory_keys_per_split(int N);                       /* 0 for N outside [1, JLM_MEMORY_MAX_KEYS] */
size_t jlm_memory_workspace_bytes(int N, int n_rows, int n_steps, int n_theta);
int jlm_memory_rows(const void *keys, const int *key_words, int N, int H, int split, float h_scale, const void *q_rows,
                    const int *q_words, int n_rows, int n_steps, const int *len, const float *thetas_host, int n_theta, float *lpm,
                    void *workspace, size_t workspace_bytes, int *flags, void *stream);

/* What a call scored against a memory has beside its jlm_score_plan (whose layout is unchanged): step t of the plan is query row t. */
typedef struct {
    const void *keys; const int *key_words; int N;    /* the memory; read only */
    void *q_rows; int *q_words;         /* [n_steps][n_rows][H] / [n_steps][n_rows] device: written by the loop, uninitialised before */
    const int *len;                     /* [n_rows] device: the steps row r is live; NULL: all */
    const float *thetas; int n_theta;   /* host */
    float *lpm;                         /* [n_theta][n_steps][n_rows] device */
    void *workspace; size_t workspace_bytes;
    int *flags;                         /* one device int or NULL: jlm_memory_rows' bit */
} jlm_memory_plan;

/* jlm_score_frames' loop -- the same launches in the same order, so nll_seq / nll_tok and the returned state are the same bits --
 * with the store hook of jlm_score_cache_frames behind every step (the live rows of the written state set into q_rows[t], the step's
 * targets into q_words[t]) and jlm_memory_rows once behind the last step.  No host synchronisation.  Every refusal of
 * jlm_memory_rows is returned before the first launch.  events as jlm_score_frames'.  Returns as jlm_score_frames does. */
int jlm_score_memory_frames(const jlm_decode_model *model_host, const jlm_score_plan *plan_host, const jlm_memory_plan *memory_host,
                            void *stream, void *const *events);

/* ------------------------------------------------------------------------
 * Exact top-K retrieval over a memory (Memory.search, jlm_amd/memory.py memory_neighbours / memory_distribution):
 * the mass of a memory on EVERY word, carried by the K nearest entries of the query.  Additive to ABI 12.
 *
 * A memory (k_i, v_i), i < N, a query state h_q, theta >= 0, 1 <= K <= JLM_MEMORY_TOPK_MAX, n_q = min(K, N), s_i = theta * (h_q . k_i)
 * as above.  T_K(q) is the n_q entries that come first in the total order "larger s_i first, smaller i first among equal s_i".  For
 * every word w
 *   c_q(w) = sum_{i in T_K, v_i = w} exp(s_i) / sum_{i in T_K} exp(s_i)
 *   p_q(w) = (1 - lambda) p_lm(w) + lambda c_q(w)             lambda = 0: p_lm, the same bits
 * With K >= N this is the distribution of the section above.  As a patch of a row's logits it is jlm_cache_mix_rows' definition below,
 * word for word, with T_K in the place of the window: rho = lambda / (1 - lambda),
 *   y'[w] = logaddexp(y[w], L + log rho + log c_q(w)) on the retrieved words, the same bits elsewhere.  One theta, lambda and K a call.
 *
 * jlm_memory_topk (csrc/jlm_memory_topk.hip: memory_topk_score_kernel, memory_topk_select_kernel):
 *   keys, key_words, N, H, split, h_scale     the memory, as jlm_memory_rows takes it
 *   q_rows    [n_rows_max][H]        one query per row -- row r < min(*n_dev, n_rows_max) is live (n_dev NULL: n_rows_max; a device
 *                                    int) -- the state rows a step just wrote, in the memory's format; rows that are not live are
 *                                    never read
 * For each live row r, entry j < n_q is the j-th of T_K, best first:
 *   s[r * ld_s + j]                  its score, f32 (ld_s >= K)
 *   ret_words[j * n_rows + r]        v_i       ([K][n_rows] int32, n_rows >= n_rows_max)
 *   ret_idx[j * n_rows + r]          i         (the same shape; may be NULL)
 * Entries j >= n_q and rows that are not live are left exactly as they were.  jlm_cache_mix_rows runs on these arrays unchanged:
 * ret_words is its words [cap][n_rows] with cap = N_window = K and pos = n_q, first a device array of zeros, s is its s.
 * Products: memory_rows_kernel's instructions in its k order -- split rows: three v_mfma_f32_32x32x16_f16 per 16 k over the stored
 * halves (hi.hi, hi.lo, lo.hi; 1 / h_scale^2 folded into theta), f32 rows: v_mfma_f32_32x32x2_f32 -- and s_i = f32(theta' * dot) + 0
 * (a zero score is +0).  The bits of s_i are a function of (query row, key row, theta) alone.
 * Selection: exact.  Scores are compared by their bits' order-preserving integer image above the complement of the index, so equal
 * score bits resolve to the smaller index and no two entries compare equal.  The memory is walked in chunks of
 * jlm_memory_topk_chunk_keys(N, n_rows_max, K, workspace_bytes) keys -- a multiple of 32, as many as the workspace holds, at most N
 * rounded up -- and a chunk's winners are merged with the running list of the earlier chunks; the result does not depend on the
 * chunk, on the row's position in the launch, on the other rows or how many are live, on what the workspace or the outputs held
 * before, or on the order any LDS counter is served in (integer counts only; no float atomics).  The workspace is
 * [n_rows_max][chunk] f32 scores and [n_rows_max][K] 8-byte list entries; jlm_memory_topk_workspace_bytes(N, n_rows_max, K) is the
 * least it may be (a chunk of 32 keys); every word of it that is read was written by the same call.
 * flags (one device int, may be NULL): |= 1 when a score of a live row is not finite.
 * Returns -1 before any launch for jlm_memory_rows' conditions on N, H, theta, h_scale, alignment (the workspace: 16 bytes) and NULL
 * pointers (n_dev, ret_idx and flags may be NULL), K outside [1, JLM_MEMORY_TOPK_MAX], ld_s < K, n_rows_max outside [0, n_rows],
 * n_rows > 65535, workspace_bytes below jlm_memory_topk_workspace_bytes(...); 0 with nothing launched for n_rows_max == 0; else 0 or
 * a hipError_t. */
#define JLM_MEMORY_TOPK_MAX 1024
size_t jlm_memory_topk_workspace_bytes(int N, int n_rows_max, int K);      /* 0 for arguments the launcher refuses */
int jlm_memory_topk_chunk_keys(int N, int n_rows_max, int K, size_t workspace_bytes);      /* 0 where the launcher refuses */
int jlm_memory_topk(const void *keys, const int *key_words, int N, int H, int split, float h_scale, const void *q_rows, int n_rows_max,
                    const int *n_dev, float theta, int K, float *s, int ld_s, int *ret_words, int *ret_idx, int n_rows, void *workspace,
                    size_t workspace_bytes, int *flags, void *stream);

/* ------------------------------------------------------------------------
 * The continuous cache on the decode side: the cache distribution over EVERY word of the window, as a patch of a row's materialised
 * logits (csrc/jlm_cache_mix.hip, jlm_amd/cache.py cache_distribution / mixed_logits).  Additive to ABI 12.
 *
 * Positions, rings, window and s_i are those of jlm_cache_rows above: the window of position q is max(q - N, first) <= i < q with n_q
 * entries, s_i = theta * (h_q . h_i) with h in real units.  For every word w
 *   c_q(w)  = sum_{i in window, w_i = w} exp(s_i) / sum_{i in window} exp(s_i)                     (0 when no i matches)
 *   p_q(w)  = (1 - lambda) p_lm(w) + lambda c_q(w)   when n_q > 0 and lambda > 0;   p_lm(w) otherwise
 *   p_lm(w) = exp(y[w] - L),  L = lse(y) over the row; self-normalised models: L = 0 (as score_fold_kernel defines nll there)
 * With rho = lambda / (1 - lambda), ordering by p_q is ordering by
 *   y'[w]   = logaddexp(y[w], L + log rho + log c_q(w))  for the words of the window;   y'[w] = y[w], the same bits, for every other
 * and lse(y') = L - log(1 - lambda): jlm_topk_rows' nll over the patched row is -log p_q(w) on ordinary models; on self-normalised
 * models the host adds -log1p(-lambda).  One theta and one lambda a call.  Rank and top-k order stay jlm_rank_rows' / jlm_topk_rows'.
 *
 * jlm_cache_query (cache_query_kernel): one query per row -- row r < min(*n_dev, n_rows_max) (n_dev NULL: n_rows_max) of q_rows
 * [.. n_rows_max][H], the state rows a step just wrote, in the rings' state-row format -- against that row's window at position
 * `pos` in hist [cap][n_rows][H] (slot = position mod cap; cap >= N, n_rows_max <= n_rows; first [n_rows] device).  Writes
 *   s[r * ld_s + j] = f32(theta' * dot),  j < n_q: window entry j, OLDEST first (position max(pos - N, first[r], 0) + j)
 * and nothing else: entries j >= n_q, rows that are not live and the rows of an empty window are left as they are.  ld_s >= N.
 * Arithmetic: split rows are decoded as f32(hi) + f32(lo) with 1 / h_scale^2 folded into theta; four lanes a key, each an f32 fmaf
 * chain in k order over the 8-value units u = lane, lane + 4, ... of the row, folded (a0 + a1) + (a2 + a3).  The bits of s[r][j] are
 * a function of the pair (h_q, h_i), H and theta alone: not of pos, cap, wrap-around, n_rows or where the key falls in the launch.
 * flags (one device int, may be NULL): |= 1 when an s inside a window is not finite.
 * Returns -1 before any launch for N < 1 or N > JLM_CACHE_MIX_MAX_N, cap < N, ld_s < N, n_rows_max outside [0, min(n_rows, 65535)],
 * H <= 0 or H % 32 != 0, theta negative or not finite, split != 0 with h_scale <= 0, pos < 0 or pos + cap >= 2^31, hist / q_rows NULL
 * or not 16-byte aligned, first / s NULL, or any of first / s / n_dev / flags not 4-byte aligned; 0 with nothing launched for
 * n_rows_max == 0; else 0 or a hipError_t. */
#define JLM_CACHE_MIX_MAX_N 4096
int jlm_cache_query(const void *hist, int cap, int n_rows, int H, int split, float h_scale, const void *q_rows, int n_rows_max,
                    const int *n_dev, int pos, const int *first, int N, float theta, float *s, int ld_s, int *flags, void *stream);

/* jlm_cache_mix_rows (cache_mix_rows_kernel, one workgroup of 256 threads per live row, 12 N bytes of LDS): rewrites, in place, row
 * r < min(*n_dev, n_rows_max) of the f32 logits y[r * ld_y + 0 .. n_cols) (jlm_topk_rows' conditions on y) into y' of the definition
 * above, from the row's scores s[r * ld_s + 0 .. n_q) (jlm_cache_query's) and the window's words in words [cap][n_rows] at `pos`.
 * Arithmetic: max, e_j = expf(s_j - max) and Z = sum e_j in a fixed tree over j; c(w) = the f32 sum of e_j over the entries with
 * w_j = w in ascending j, formed at the FIRST occurrence of w in the window (one writer per word, no atomics); L as jlm_topk_rows
 * forms its lse (f32 expf, f64 sums, its order), rounded to f32, 0 on self_norm models;
 *   y'[w] = logaddexp_f32(y[w], (L + logf(rho)) + (logf(c) - logf(Z)))      y[w] = -inf: the cache term itself
 * y' is a function of the window's contents in order (s_j, w_j), the row and lambda alone: the same bits for any cut of a stream, any
 * pos / cap / wrap-around and whatever else the launch carries.  Every word outside the window keeps its bits.
 * lpc_ent (may be NULL) [.. n_rows_max][ld_s]: logf(c(w_j)) - logf(Z) at j when entry j is the first occurrence of its word, -inf
 * at a repeat; written for the rows that are patched, j < n_q.
 * flags (one device int, may be NULL): |= 1 a row whose window holds an s that is not finite, |= 2 a row whose L is not finite (a
 * NaN or +inf logit, or none above -inf): such a row is left exactly as it is.  |= 4 a window word outside [0, n_cols): the entry
 * counts in Z, patches nothing, and nothing is indexed by it; the row's other words are patched.  A NaN y[w] stays NaN.
 * lambda == 0 launches nothing; an empty window leaves the row's bits.
 * Returns -1 before any launch for lambda outside [0, 1), the conditions of jlm_cache_query on N, cap, ld_s, n_rows_max, pos, first,
 * n_dev and flags, jlm_topk_rows' on y / ld_y / n_cols, s or words NULL, or s / words / lpc_ent not 4-byte aligned; else 0 or a
 * hipError_t. */
int jlm_cache_mix_rows(float *y, int ld_y, int n_cols, int self_norm, const float *s, int ld_s, const int *words, int cap, int n_rows,
                       int n_rows_max, const int *n_dev, int pos, const int *first, int N, float lam, float *lpc_ent, int *flags,
                       void *stream);

/* What a cached ranking call has beside its jlm_rank_plan (whose layout is unchanged): the rings of jlm_cache_rows over the plan's
 * n_rows rows, step t of the plan being position pos0 + t; cap >= N (the slot a step writes left every later window N steps ago). */
typedef struct {
    void *hist; int *words; int cap;    /* the rings; the entries carried into the call are in their slots already */
    int pos0;                           /* the position of step 0 */
    const int *first;                   /* [n_rows] device */
    int N;
    float theta, lam;
    float *s; int ld_s;                 /* [n_rows][ld_s] device scratch: the scores of one step, ld_s >= N */
    int top_k;                          /* 0: no lists */
    int *top_ids; double *top_nll;      /* [n_steps][n_rows][top_k] device: jlm_topk_rows over the patched rows of every step */
    int *flags;                         /* one device int or NULL: the bits of jlm_cache_query / jlm_cache_mix_rows */
} jlm_cache_mix_plan;

/* jlm_rank_frames' loop -- the same launches in the same order -- with, per step, between the logit GEMMs and the ranking,
 * jlm_cache_query on the state set the step wrote at position pos0 + t and jlm_cache_mix_rows on the logits, so that rank_rows_kernel
 * ranks target[t] under the mixed distribution; behind the ranking, with top_k > 0, jlm_topk_rows over the n_live_host[t] live rows
 * into top_ids / top_nll (n_live_host is required then; its flags go to the rank plan's), and jlm_cache_store of the written state
 * rows and the step's targets into slot (pos0 + t) mod cap: the rings hold what jlm_score_cache_frames would have put there.
 * No host synchronisation.  Every refusal of the two launchers (at the call's last position), top_k outside 0 .. min(JLM_TOPK_MAX,
 * V), and an n_live_host[t] outside [0, n_rows] is returned before the first launch.  events (may be NULL):
 * JLM_RANK_CACHE_EVENTS_PER_STEP * n_steps hipEvent_t, [0] .. [3] as jlm_rank_frames', [4] after the query, [5] after the patch,
 * [6] after the ranking, the lists and the ring write.  Returns as jlm_rank_frames does. */
#define JLM_RANK_CACHE_EVENTS_PER_STEP 7
int jlm_rank_cache_frames(const jlm_decode_model *model_host, const jlm_rank_plan *plan_host, const jlm_cache_mix_plan *cache_host,
                          void *stream, void *const *events);

/* One step of prediction under the cache, for a caller who holds the carried state of n_rows streams and their rings. */
typedef struct {
    int n_rows;
    const void *h;                      /* [n_rows, H] the carried state rows, in the model's state-row format */
    float *T;                           /* [n_rows, ldt] f32 scratch (an untied f32 model: unused, T is h) */
    float *logits; int ld_logits;       /* [n_rows, ld_logits] f32 scratch, ld_logits >= V rounded up to 4 */
    const int *rows;                    /* [n_rows] device: 0, 1, ..., n_rows - 1 */
    const void *hist; const int *words; int cap;    /* the rings [cap][n_rows][..] */
    int pos;                            /* the position of the streams' next step */
    const int *first;                   /* [n_rows] device */
    int N;
    float theta, lam;
    float *s; int ld_s;                 /* [n_rows][ld_s] device scratch */
    int k;                              /* 1 .. min(JLM_TOPK_MAX, V) */
    const unsigned *mask; int ld_mask, n_sets; const int *row_set;    /* jlm_topk_rows_masked's; row_set NULL: jlm_topk_rows */
    int *ids; double *nll;              /* [n_rows][k] device */
    int *flags;                         /* one device int or NULL: the selection's */
    int *cache_flags;                   /* one device int or NULL: the bits of jlm_cache_query / jlm_cache_mix_rows */
} jlm_predict_cache_plan;

/* Enqueues the T projection of h, the logit GEMMs, jlm_cache_query at pos, jlm_cache_mix_rows and jlm_topk_rows (row_set: _masked):
 * ids / nll are the k best words of every row under the mixed distribution (self_norm models: the host adds -log1p(-lambda) where
 * the window is not empty).  No LSTM step, no ring write, no host synchronisation; every refusal before the first launch.  Returns
 * -2 for an untied split-row model -- its vocabulary GEMMs read the f32 copy of the state that only the LSTM step writes -- and
 * otherwise as the launchers do. */
int jlm_predict_cache_rows(const jlm_decode_model *model_host, const jlm_predict_cache_plan *plan_host, void *stream);

/* What a ranking call under a memory has beside its jlm_rank_plan (whose layout is unchanged): the memory, one theta / lambda / K, and
 * the retrieval's buffers over the plan's n_rows rows (jlm_memory_topk's, above). */
typedef struct {
    const void *keys; const int *key_words; int N;    /* the memory; read only */
    float theta, lam; int K;
    float *s; int ld_s;                 /* [n_rows][ld_s] device scratch: the scores of one step's neighbours, ld_s >= K */
    int *ret_words;                     /* [K][n_rows] device scratch: their words */
    int *ret_idx;                       /* [K][n_rows] device scratch, or with keep_idx != 0 [n_steps][K][n_rows]: every step's indices */
    int keep_idx;
    const int *first;                   /* [n_rows] device zeros: jlm_cache_mix_rows' `first` */
    void *workspace; size_t workspace_bytes;
    int top_k;                          /* 0: no lists */
    int *top_ids; double *top_nll;      /* [n_steps][n_rows][top_k] device: jlm_topk_rows over the patched rows of every step */
    int *flags;                         /* one device int or NULL: the bits of jlm_memory_topk / jlm_cache_mix_rows */
} jlm_memory_mix_plan;

/* jlm_rank_frames' loop -- the same launches in the same order -- with, per step, between the logit GEMMs and the ranking,
 * jlm_memory_topk on the state set the step wrote and jlm_cache_mix_rows on the logits (words = ret_words, cap = N_window = K,
 * pos = min(K, N)), so that rank_rows_kernel ranks target[t] under p_q of the section "Exact top-K retrieval" above; behind the
 * ranking, with top_k > 0, jlm_topk_rows over the n_live_host[t] live rows (n_live_host is required then; its flags go to the rank
 * plan's).  Nothing is written to the memory and no ring is kept.  No host synchronisation.  Every refusal of the two launchers,
 * top_k outside 0 .. min(JLM_TOPK_MAX, V) and an n_live_host[t] outside [0, n_rows] is returned before the first launch.  events (may
 * be NULL): JLM_RANK_MEMORY_EVENTS_PER_STEP * n_steps hipEvent_t, [0] .. [3] as jlm_rank_frames', [4] after the retrieval, [5] after
 * the patch, [6] after the ranking and the lists.  Returns as jlm_rank_frames does. */
#define JLM_RANK_MEMORY_EVENTS_PER_STEP 7
int jlm_rank_memory_frames(const jlm_decode_model *model_host, const jlm_rank_plan *plan_host, const jlm_memory_mix_plan *memory_host,
                           void *stream, void *const *events);

/* One step of prediction under a memory, for a caller who holds the carried state of n_rows streams. */
typedef struct {
    int n_rows;
    const void *h;                      /* [n_rows, H] the carried state rows, in the model's state-row format */
    float *T;                           /* [n_rows, ldt] f32 scratch (an untied f32 model: unused, T is h) */
    float *logits; int ld_logits;       /* [n_rows, ld_logits] f32 scratch, ld_logits >= V rounded up to 4 */
    const int *rows;                    /* [n_rows] device: 0, 1, ..., n_rows - 1 */
    const void *keys; const int *key_words; int N;
    float theta, lam; int K;
    float *s; int ld_s; int *ret_words; int *ret_idx;      /* jlm_memory_topk's outputs over n_rows rows; ret_idx may be NULL */
    const int *first;                   /* [n_rows] device zeros */
    void *workspace; size_t workspace_bytes;
    int k;                              /* 1 .. min(JLM_TOPK_MAX, V) */
    const unsigned *mask; int ld_mask, n_sets; const int *row_set;    /* jlm_topk_rows_masked's; row_set NULL: jlm_topk_rows */
    int *ids; double *nll;              /* [n_rows][k] device */
    int *flags;                         /* one device int or NULL: the selection's */
    int *memory_flags;                  /* one device int or NULL: the bits of jlm_memory_topk / jlm_cache_mix_rows */
} jlm_predict_memory_plan;

/* jlm_predict_cache_rows with the retrieval in the query's place: the T projection of h, the logits, jlm_memory_topk, the patch and
 * jlm_topk_rows (row_set: _masked).  No LSTM step, no host synchronisation; every refusal before the first launch.  Returns -2 for an
 * untied split-row model, for jlm_predict_cache_rows' reason, and otherwise as the launchers do. */
int jlm_predict_memory_rows(const jlm_decode_model *model_host, const jlm_predict_memory_plan *plan_host, void *stream);

/* ------------------------------------------------------------------------
 * Left context of a decode (LSTM_Model.prime, Decoder.decode(context=), jlm_amd/context.py).  Sentence s with the committed words
 * ctx_s has the history hist = [<eos>] + ctx_s; its decode is the reference's with the root hypothesis consuming hist[-1] from the
 * state reached by consuming hist[:-1] from the zero state.
 *
 * The priming loop: row r < n_rows consumes its words RIGHT-aligned on n_steps frames, rows sorted longest first, as
 * jlm_generate_plan's prompt frames: frame f steps the live prefix r < n_live[f], consuming word[f][r] and continuing row prev[f][r]
 * of the set being read (-1 at a row's first frame: the zero state).  State h[2] / c[2] ping-pong as jlm_score_plan's: the state
 * after the last frame is in set n_steps % 2.  A row without words never steps (its state rows are not written). */
typedef struct {
    int n_rows, n_steps;
    void *h[2]; float *c[2];        /* [n_rows, H] state row sets */
    const int *rows;                /* [n_rows] device: 0, 1, ..., n_rows - 1 */
    const int *prev, *word;         /* [n_steps][n_rows] device */
    const int *n_live;              /* [n_steps] device */
    const int *n_live_host;         /* [n_steps] host */
} jlm_prime_plan;

/* Enqueues n_steps LSTM steps and nothing else (jlm_lstm_step_xg on split-row models, jlm_lstm_step otherwise; no f32 copy of the
 * state, no T projection, no normaliser, no host synchronisation).  Returns 0, -2 for a model outside the loop's shapes, -1 / a
 * hipError_t as the launchers do. */
int jlm_prime_frames(const jlm_decode_model *model_host, const jlm_prime_plan *plan_host, void *stream);

/* Seeds a decode plan with primed states (seed_context_kernel, one launch, plain vector stores).  For sentence s < n_sent with
 * r = idx[s] (a row of the primed set, 0 <= r < n_src; a sentence with r outside that range is left alone):
 *   has[r] != 0: rows r of src_h / src_c -> rows G + s of dst_h / dst_c, as H / 4 16-byte records each (the state-row format of the
 *                model, split or f32, is copied as it is), and ctx_prev[s * beam] = G + s;
 *   has[r] == 0: (the history is <eos> alone) nothing is copied, ctx_prev[s * beam] = -1;
 *   ctx_word[s * beam] = last[r].
 * Entries of ctx_prev / ctx_word at other positions are not written.  H % 4 == 0; every pointer 16-byte aligned; (G + n_sent) x H / 4
 * < 2^31 (the LSTM step's addressing).  Returns 0, -1 for bad arguments, or a hipError_t. */
int jlm_seed_context(const void *src_h, const float *src_c, int H, const int *last, const int *has, int n_src, const int *idx,
                     int n_sent, int beam, long long G, void *dst_h, float *dst_c, int *ctx_prev, int *ctx_word, void *stream);

/* ------------------------------------------------------------------------
 * The continuous cache inside a decode (Decoder.decode(context=, cache=); ABI 12, additive).  Sections 18 / 20's
 * definition with a window that is FIXED for the whole decode: sentence s with hist = [<eos>] + ctx_s has the window of the last
 * n_s = min(len(ctx_s), N) pairs (h_j, hist[j + 1]), h_j the state after consuming hist[j] from the zero state -- the state that
 * predicted hist[j + 1]; a decode's own hypotheses add nothing.  For hypothesis row r of sentence s in frame f, with the state h_r the
 * frame's LSTM step wrote, and every lattice word w that starts in cell (f, s):
 *     s_i    = theta (h_r . h_i)                         i in the window of s, h in real units
 *     c_r(w) = sum_{i : w_i = w} exp(s_i) / sum_i exp(s_i)
 *     p_r(w) = (1 - lam) p_lm(w | r) + lam c_r(w)        if n_s > 0;  p_lm(w | r) if n_s = 0
 *     edge cost = -log p_r(w),   p_lm = exp(y - L), L the row's full-vocabulary log-normaliser (self-normalised models: 0).
 * Word ids are only compared (an out-of-vocabulary lattice word is id 0 and mixes like any other).  One theta and one lam a call,
 * N <= JLM_CACHE_MIX_MAX_N.  The beam step computes score + (lse - edge) in f64, so the feature is a rewrite of the edge buffer:
 *     edge' = L + log(1 - lam) + logaddexp(y - L, log rho + log M - log Z)   for a word with a match (rho = lam / (1 - lam)),
 *     edge' = y + log(1 - lam)                                              for a word without,
 * formed in f64 from the f32 sums M = sum_{i : w_i = w} e_i and Z = sum_i e_i, e_i = expf(s_i - max s), and rounded once to the f32
 * the buffer holds.  Rows of a sentence with n_s = 0 keep their bits.
 *
 * The window of cache row r (rows of a CachedContext, jlm_amd/context.py): hist [cap][n_src][H] in the model's state-row format,
 * words [cap][n_src], count [n_src] <= cap; its entries are the slots cap - count[r] .. cap - 1, oldest first.  Slots below that
 * are never read.  idx [n_sent]: the cache row of every sentence of the batch (outside [0, n_src): no window). */
typedef struct jlm_decode_cache {
    const void *hist; const int *words, *count; int cap, n_src;
    const int *idx;                 /* [n_sent] device */
    int N; float theta, lam;
    float *s; int ld_s;             /* scratch [n_sent * beam][ld_s], ld_s >= min(cap, N); contents arbitrary */
} jlm_decode_cache;

/* cache_cell_query_kernel: s[(j * beam + k) * ld_s + i] = theta (h[g0[j] + k] . key_i) for every sentence j < n_sent with
 * frame < sent_len[j], slot k < min(cnt[j], beam) and entry i < n_j = min(count[idx[j]], cap, N) of its window (oldest first).
 * Grid (chunk of 64 keys, sentence): the cell's query rows are staged in LDS eight at a time and every key of the chunk is dotted
 * against each; per (query, key) the partition, the f32 fmaf chain, the reduction and the decode of split rows are jlm_cache_query's,
 * so the bits are its bits for the same two rows and theta, whatever the cell, the chunk, cnt or the launch.  g0, cnt [n_sent]: the
 * frame's entries (jlm_decode_plan.g0 + cell, jlm_beam_state.cnt + cell).  A product that is not finite ORs 8 into *flags.
 * Returns 0, -1 for bad arguments (H % 32, H > 2048 -- the staged rows take 32 H bytes of LDS --, N outside [1, JLM_CACHE_MIX_MAX_N], cap < 1, ld_s < min(cap, N), theta, h_scale, a null
 * or misaligned pointer, n_sent > 65535) before any launch, or a hipError_t. */
int jlm_cache_cell_query(const void *h, int H, int split, float h_scale, const int *g0, const int *cnt, const int *sent_len, int frame,
                         int n_sent, int beam, const void *hist, const int *count, int cap, int n_src, const int *idx, int N,
                         float theta, float *s, int ld_s, int *flags, void *stream);

/* cache_cell_patch_kernel: one workgroup per sentence j of the frame (skipped when frame >= sent_len[j] or cnt[j] = 0).
 * part != NULL (ordinary models): the (max, sum exp) slices part[p * ld_part + live_base[j] + k], p < n_parts, of the cell's rows
 * are first folded into lse[j * beam + k] (f64) with jlm_beam_step's fused fold -- its order, arithmetic and sanitising: a value
 * that is not finite ORs 1 into *flags and becomes 1e30 -- whether the sentence has a window or not, so that the next jlm_beam_step
 * runs in its unfused form; part == NULL (self-normalised models): L = 0, lse is not touched.  Then, for a sentence with n_j > 0:
 * per slot the maximum, e_i = expf(s_i - max) (written back over s) and Z in a fixed tree; per position of the cell's word list
 * wl[wl_off[l] .. wl_off[l + 1]), l = wl_base + wl_idx[j] (jlm_edge_logits' lists, found as it finds them) and slot k, M in ascending
 * i and edge[wl_out * beam + k] <- edge' as defined above.  One writer per address, no atomics.  A slot with a score that is not
 * finite keeps its edge logits (8 is ORed into *flags).  lse, g-indexed arrays: the frame's first entry.
 * Returns 0, -1 for bad arguments (lam outside (0, 1), N, cap, ld_s, beam outside [1, JLM_MAX_BEAM], part without live_base / lse /
 * n_parts >= 1, a null pointer) before any launch, -3, or a hipError_t. */
int jlm_cache_cell_patch(float *s, int ld_s, const int *words, const int *count, int cap, int n_src, const int *idx, int N, float lam,
                         const int *cnt, const int *sent_len, int frame, int n_sent, int beam, const int *wl, const int *wl_off,
                         const int *wl_idx, int wl_base, const int *wl_out, float *edge, const float *part, int ld_part, int n_parts,
                         const int *live_base, double *lse, int *flags, void *stream);

/* ------------------------------------------------------------------------
 * A back-off word n-gram model mixed into a decode (Decoder.decode(ngram=); ABI 12, additive).
 *
 * Table: tuples of 1 .. order word ids, order 1, 2 or 3, -> (lp, bow): lp the natural log of the conditional probability of the
 * tuple's last word, bow the natural log of the back-off weight of the tuple as a context (0 where the file gives none); both the
 * float32 nearest to ln 10 x the file's number, everything after that float64.  Word ids <= 2^21 - 2, lp <= 0, both finite: the
 * host refuses anything else when it builds the table (jlm_amd/ngram.py), so the kernel has no flag for it.
 * For a history h = (.., u, v) and a word w, with k = min(order - 1, len(h)) history words in use:
 *     q(w | h_k) = lp(h_k, w)                                 if (h_k, w) is in the table
 *                = -inf                                       else if k = 0   (a word without a unigram: p_ng = 0)
 *                = bow(h_k) [0 if absent] + q(w | h_{k-1})    else            (h_{k-1} drops the oldest word)
 * -- ARPA back-off with the weights applied.  The history of a hypothesis is [<eos>] + context + the path's words so far: a decode
 * without context starts from (<eos>) alone, its first word is predicted from the bigram (<eos>, w), never from a padded trigram.
 * For hypothesis row r with full-vocabulary log-normaliser L (self-normalised models: 0) and every lattice word w leaving its cell,
 * with logit y:
 *     p_r(w) = (1 - lam) exp(y - L) + lam exp(q(w | hist_r)),     0 < lam < 1, one lam a call
 *     edge'  = L + log(1 - lam) + logaddexp(y - L, log(lam / (1 - lam)) + q)      q finite
 *     edge'  = y + log(1 - lam)                                                  q = -inf
 * formed in f64 and rounded once to the f32 the buffer holds.  Word ids are only compared; the raw-kana fallback is id 0 and mixes
 * like any other word.
 *
 * The table on the device: keys [2^log2cap] 64-bit, vals [2^log2cap][2] float32 (lp, bow).  key = (w + 1) | (v + 1) << 21 |
 * (u + 1) << 42 with the predicted word lowest and absent positions 0 -- key 0 is an empty slot; home slot
 * (key * 0x9E3779B97F4A7C15) >> (64 - log2cap), linear probing; max_probe the longest displacement in use.  A probe stops on the
 * key, on 0, or after max_probe + 1 slots.  root_hist [n_sent][2]: the last two words of [<eos>] + context of every sentence of the
 * batch, -1 for "no word". */
typedef struct jlm_decode_ngram {
    const void *keys; const float *vals; int log2cap, max_probe, order; float lam;
    const int *root_hist;           /* [n_sent][2] device */
} jlm_decode_ngram;

/* ngram_cell_patch_kernel (csrc/jlm_ngram_edge.hip): one workgroup per sentence j of the frame (skipped when frame >= sent_len[j] or
 * cnt[j] = 0).  part != NULL: the cell's normaliser slices are first folded into lse[j * beam + k] exactly as jlm_cache_cell_patch
 * folds them (jlm_beam_step's fused fold: order, arithmetic, sanitising -- flag bit 1, the value 1e30), so that the next
 * jlm_beam_step runs unfused; part == NULL: L = 0, lse is not touched.  Slot k < min(cnt[j], beam) is row g = g0[j] + k of the
 * pools bp / word / score (jlm_beam_state's, whole): its newest word is word[g], the one before word[bp[g]]; where the walk reaches
 * a root (bp = -1) the words come from root_hist[j] -- a root row's own word is never read.  Per position of the cell's word list
 * wl[wl_off[l] .. wl_off[l + 1]), l = wl_base + wl_idx[j] (jlm_edge_logits' lists) and slot k: edge[wl_out * beam + k] <- edge'.
 * One writer per address.  A slot whose score[g] is not finite (score may be NULL: not looked at) keeps its edge logits and ORs 8
 * into *flags.  lse: the frame's first entry.
 * Returns 0, -1 before any launch (order outside 1 .. 3, log2cap outside 6 .. 31, max_probe >= 2^log2cap, lam outside (0, 1), beam
 * outside [1, JLM_MAX_BEAM], a null or misaligned pointer, part without live_base / lse / n_parts >= 1), or a hipError_t. */
int jlm_ngram_cell_patch(const void *keys, const float *vals, int log2cap, int max_probe, int order, float lam, const int *g0,
                         const int *cnt, const int *sent_len, int frame, int n_sent, int beam, const int *bp, const int *word,
                         const double *score, const int *root_hist, const int *wl, const int *wl_off, const int *wl_idx, int wl_base,
                         const int *wl_out, float *edge, const float *part, int ld_part, int n_parts, const int *live_base, double *lse,
                         int *flags, void *stream);

/* ------------------------------------------------------------------------
 * A memory of (hidden state, next word) pairs inside a decode (Decoder.decode(memory=); ABI 12, additive): the
 * distribution of jlm_memory_topk's section above on the edges of the continuous cache's section.  A memory (k_i, v_i), i < N; one
 * theta >= 0, one 0 < lam < 1 and one 1 <= K <= JLM_MEMORY_TOPK_MAX a call; n_q = min(K, N).  For hypothesis row r of sentence s in
 * frame f, with the state h_r the frame's LSTM step wrote and T_K(r) the retrieval's set for the query h_r (its total order: larger
 * s_i = theta (h_r . k_i) first, smaller i first among equal s_i), and every lattice word w that starts in cell (f, s):
 *     c_r(w) = sum_{i in T_K(r), v_i = w} exp(s_i) / sum_{i in T_K(r)} exp(s_i)
 *     p_r(w) = (1 - lam) p_lm(w | r) + lam c_r(w)
 *     edge'  = L + log(1 - lam) + logaddexp(y - L, log rho + log M - log Z)   for a word with a match (rho = lam / (1 - lam)),
 *     edge'  = y + log(1 - lam)                                              for a word without,
 * formed in f64 from the f32 sums M = sum_{i : v_i = w} e_i and Z = sum_i e_i over the retrieved list, e_i = expf(s_i - max s), and
 * rounded once to the f32 the buffer holds: cache_cell_patch_kernel's arithmetic, operation for operation -- lane-strided partial sums
 * for Z, then the xor-shuffle tree; M in ascending list position; the same logaddexp.  L is the row's full-vocabulary log-normaliser
 * (self-normalised models: 0).  Word ids are only compared.  A decode's own hypotheses add nothing to the memory.  The memory applies
 * with or without a left context, and to every row: a memory is never empty.
 *
 * What the frame loop is handed: the memory as jlm_memory_topk takes it, and the buffers of one frame's retrieval over the
 * n_rows = n_sent * beam rows of the batch -- q_rows [n_rows][H], the frame's live rows gathered (jlm_memory_gather_rows), then
 * jlm_memory_topk's s / ret_words / workspace.  flags: the retrieval's own flag int (its bit 0, a score that is not finite, would
 * collide with bit 0 of the batch's word); the patch flags in jlm_beam_state.flags as the cache's patch does.  Per frame, behind the
 * normaliser: gather, jlm_memory_topk (n_dev = the frame's live count), patch. */
typedef struct jlm_decode_memory {
    const void *keys; const int *key_words; int N, K; float theta, lam;
    void *q_rows;                   /* [n_sent * beam][H] in the model's state-row format, 16-byte aligned; contents arbitrary */
    float *s; int ld_s;             /* [n_sent * beam][ld_s], ld_s >= K */
    int *ret_words;                 /* [K][n_sent * beam] */
    void *workspace; size_t workspace_bytes;       /* jlm_memory_topk's, for n_rows_max = n_sent * beam */
    int *flags;                     /* one device int or NULL: jlm_memory_topk's bits */
} jlm_decode_memory;

/* memory_gather_rows_kernel: for i < min(*n_dev, n_rows_max) (n_dev NULL: n_rows_max), row rows[i] of the pool h [n_pool_rows][H]
 * -> row i of out [n_rows_max][H]; a row is 4 H bytes in either state-row format and moves as 16-byte records.  Rows of out that are
 * not live are not written; an index outside [0, n_pool_rows) copies nothing.
 * Returns 0 (nothing launched for n_rows_max == 0), -1 before any launch (H <= 0 or H % 4, n_rows_max outside [0, 65535], a null
 * pointer, h or out off 16 bytes), or a hipError_t. */
int jlm_memory_gather_rows(const void *h, int H, long long n_pool_rows, const int *rows, const int *n_dev, int n_rows_max, void *out,
                           void *stream);

/* memory_cell_patch_kernel (csrc/jlm_memory_edge.hip): one workgroup per sentence j of the frame (skipped when frame >= sent_len[j]
 * or cnt[j] = 0).  part != NULL: the cell's normaliser slices are first folded into lse[j * beam + k] exactly as jlm_cache_cell_patch
 * folds them (jlm_beam_step's fused fold: order, arithmetic, sanitising -- flag bit 1, the value 1e30), so that the next jlm_beam_step
 * runs unfused; part == NULL: L = 0, lse is not touched.  Slot k < min(cnt[j], beam) is compact row c = live_base[j] + k of the
 * frame's live rows -- the indexing of the normaliser's slices --: its scores are s[c * ld_s + i], its words ret_words[i * n_rows + c],
 * i < n_q = min(K, N), jlm_memory_topk's outputs; entries i >= n_q are never read.  Per position of the cell's word list
 * wl[wl_off[l] .. wl_off[l + 1]), l = wl_base + wl_idx[j] (jlm_edge_logits' lists) and slot k: edge[wl_out * beam + k] <- edge' as
 * defined above.  Every slot has its own words: no match structure is shared within a cell.  One writer per address, no float
 * atomics; s and ret_words are only read.  A slot with a score that is not finite keeps its edge logits and ORs 8 into *flags.  lse:
 * the frame's first entry.  LDS: 32 bytes an entry of the list (n_q rounded up to a multiple of 4: 32 KiB at K = 1 024), whatever the beam.
 * Returns 0, -1 before any launch (lam outside (0, 1), N < 1, K outside [1, JLM_MEMORY_TOPK_MAX], ld_s < K, n_rows outside
 * [1, 65535], beam outside [1, JLM_MAX_BEAM], n_sent > 65535, part without lse / n_parts >= 1, a null or misaligned pointer), or a
 * hipError_t. */
int jlm_memory_cell_patch(const float *s, int ld_s, const int *ret_words, int n_rows, int N, int K, float lam, const int *cnt,
                          const int *sent_len, int frame, int n_sent, int beam, const int *wl, const int *wl_off, const int *wl_idx,
                          int wl_base, const int *wl_out, float *edge, const float *part, int ld_part, int n_parts, const int *live_base,
                          double *lse, int *flags, void *stream);

/* ------------------------------------------------------------------------
 * The n-gram model's distribution over EVERY word of a row, as a patch of the row's materialised logits (ABI 12,
 * additive), so that rank_rows_kernel, topk_rows_kernel and topk_rows_masked_kernel run unchanged on the mixture.  q(w | h) is the
 * definition above.  A row has f32 logits y[0 .. V), the history (u, v) = hist[r] (-1: no word; v = -1: no history at all) and
 * L = lse(y) in topk_rows_kernel's arithmetic (self_norm: 0), read before any word is patched:
 *     y'[w] = logaddexp(y[w], L + log(lam / (1 - lam)) + q(w | h))     q finite (y[w] = -inf: the finite n-gram term)
 *     y'[w] = y[w], the same bits                                      q = -inf
 * so that (1 - lam) exp(y' - L) is the mixture; the selection kernels report lse(y') - y', -log of the ROW-NORMALISED mixture (equal
 * to the mixture for a table that sums to one), and -y' on self-normalised models, where the host adds -log1p(-lam).
 *
 * The table for this walk (jlm_amd/ngram.py NGramTable.successor_arrays): dense unigrams uni_lp [V] (-inf: none) and uni_bow [V];
 * bigrams in CSR by context word, bi_off [V + 1] into bi_w / bi_lp [n_bi]; trigrams in CSR by context index, tri_off [n_ctx + 1] into
 * tri_w / tri_lp [n_tri], and tri_bow [n_ctx] = bow(u v); the context index of (u, v) is found in an open-addressing map ctx_keys
 * [2^log2cap] 64-bit / ctx_vals [2^log2cap], key (v + 1) | (u + 1) << 21, key 0 an empty slot, the hash and the probing of
 * jlm_decode_ngram's table: a hit in the home slot is one round trip. */
typedef struct jlm_ngram_rows {
    const float *uni_lp, *uni_bow;
    const int *bi_off, *bi_w; const float *bi_lp; int n_bi;
    const int *tri_off, *tri_w; const float *tri_lp, *tri_bow; int n_tri, n_ctx;
    const void *ctx_keys; const int *ctx_vals; int log2cap, max_probe;
} jlm_ngram_rows;

/* ngram_mix_rows_kernel (csrc/jlm_ngram_mix.hip): one workgroup of 256 threads per live row r < min(n_rows, *n_dev) (n_dev may be
 * NULL), (V + 31) / 32 * 4 bytes of LDS for a bitmap of the patched words.  The trigram successors of (u, v) are patched with
 * q = lp, then the bigram successors of v that no trigram covered with q = bow(u v) + lp, then every remaining word with a unigram
 * with q = (bow(u v) + bow(v)) + lp, all in f32: t = (L + logf(rho)) + q, y' = max + log1pf(expf(min - max)).  order = 1 or v = -1:
 * the last pass alone; order = 2 or u = -1: the last two.  The bitmap (integer OR in LDS) gives every logit one writer, which reads
 * the original y[w]; no float atomics, plain vector loads and stores.  Every index read from a table array -- a range bound, a
 * context index, a successor word -- is checked against n_bi / n_tri / n_ctx / V before it is used (a bad one is skipped), every
 * probe loop ends after max_probe + 1 slots and every slot is masked into the map, whatever the table holds.  The bytes of y'[r] are
 * a function of y[r][0 .. V), hist[r] and the table: not of n_rows, r, or what lies beyond V or beyond the live rows, where nothing
 * is written.  *flags (may be NULL) |= 2: L of a row is not finite, |= 4: a history id outside [-1, V); the row is left as it is.
 * Returns -1 before any launch for order outside 1 .. 3, lam outside (0, 1), V < 1 or V > JLM_NGRAM_MIX_MAX_V (the bitmap's LDS),
 * ld_y % 4 != 0 or ld_y < V rounded up to 4, negative n_rows / n_bi / n_tri / n_ctx, log2cap outside 6 .. 31, max_probe outside
 * [0, 2^log2cap), a null pointer, y not 16-byte, ctx_keys not 8-byte or another pointer not 4-byte aligned;
 * 0 for n_rows = 0; a hipError_t of the launch.  jlm_ngram_mix_refuse: the refusals on their own. */
#define JLM_NGRAM_MIX_MAX_V 393216      /* 48 KB of bitmap, beside under 100 bytes of static LDS: inside the 64 KB a workgroup
                                         * may ask for without an attribute */
int jlm_ngram_mix_refuse(const float *y, int ld_y, int n_cols, const jlm_ngram_rows *table, const int *hist, int n_rows, const int *n_dev,
                         float lam, int order, const int *flags);
int jlm_ngram_mix_rows(float *y, int ld_y, int n_cols, int self_norm, const jlm_ngram_rows *table, const int *hist, int n_rows,
                       const int *n_dev, float lam, int order, int *flags, void *stream);

/* ngram_hist_advance_kernel: hist_out[q] = (hist_in[prev_row[q]][1], word[q]) for q < n -- the histories of the rows a beam merge
 * wrote, from those of the rows it chose them from; hist_in and hist_out are different buffers (double-buffered by the caller).  A
 * prev_row outside [0, n_in): (-1, word[q]).  Returns -1 for negative n / n_in, a null or misaligned pointer or hist_in == hist_out. */
int jlm_ngram_hist_advance(const int *hist_in, int n_in, const int *prev_row, const int *word, int n, int *hist_out, void *stream);

/* What a ranking call under the n-gram mixture has beside its jlm_rank_plan (whose layout is unchanged). */
typedef struct {
    const jlm_ngram_rows *table; int order; float lam;
    const int *hist;                    /* [n_steps][n_rows][2] device: (u, v) before target[t][r]; the loop is teacher-forced */
    int top_k;                          /* 0: no lists */
    int *top_ids; double *top_nll;      /* [n_steps][n_rows][top_k] device: jlm_topk_rows over the patched rows of every step */
    int *flags;                         /* one device int or NULL: the bits of jlm_ngram_mix_rows */
} jlm_ngram_mix_plan;

/* jlm_rank_frames' loop -- the same launches in the same order -- with, per step, between the logit GEMMs and the ranking,
 * jlm_ngram_mix_rows on the step's live rows with the histories hist[t], so that rank_rows_kernel ranks target[t] under the mixture;
 * behind the ranking, with top_k > 0, jlm_topk_rows over the n_live_host[t] live rows into top_ids / top_nll (n_live_host is required
 * then; its flags go to the rank plan's).  No host synchronisation.  Every refusal of jlm_ngram_mix_rows, top_k outside 0 ..
 * min(JLM_TOPK_MAX, V) and an n_live_host[t] outside [0, n_rows] is returned before the first launch.  events (may be NULL):
 * JLM_RANK_NGRAM_EVENTS_PER_STEP * n_steps hipEvent_t, [0] .. [3] as jlm_rank_frames', [4] after the patch, [5] after the ranking
 * and the lists.  Returns as jlm_rank_frames does. */
#define JLM_RANK_NGRAM_EVENTS_PER_STEP 6
int jlm_rank_ngram_frames(const jlm_decode_model *model_host, const jlm_rank_plan *plan_host, const jlm_ngram_mix_plan *ngram_host,
                          void *stream, void *const *events);

/* What a completion under the n-gram mixture has beside its jlm_complete_plan (whose layout is unchanged): hist[0] and hist[1], two
 * different 8-byte aligned device buffers [n_prompts * beam][2].  hist[0][p] = the last two words of prompt p (-1: no word), from the
 * host; selecting frame k reads hist[k & 1] and, behind its merge, writes hist[(k + 1) & 1] (jlm_ngram_hist_advance over the rows the
 * merge wrote; not behind the last).  hist[1] is not looked at when n_words = 1. */
typedef struct {
    const jlm_ngram_rows *table; int order; float lam;
    int *hist[2];
    int *flags;                         /* one device int or NULL: the bits of jlm_ngram_mix_rows */
} jlm_complete_ngram_plan;

/* jlm_complete_frames (prompt_set NULL; then mask NULL and n_sets 0) or jlm_complete_frames_masked (prompt_set given) -- the same
 * launches in the same order -- with jlm_ngram_mix_rows on the n_sel rows of every selecting frame between the logit GEMMs and the
 * selection, and the history advance behind every merge: a hypothesis is continued under the mixture of its own last two words.
 * Every refusal before the first launch; no host synchronisation; events as jlm_complete_frames' (the patch is inside the selection's
 * bracket, the advance inside the merge's). */
int jlm_complete_frames_ngram(const jlm_decode_model *model_host, const jlm_complete_plan *plan_host,
                              const jlm_complete_ngram_plan *ngram_host, const unsigned *mask, int ld_mask, int n_sets,
                              const int *prompt_set, void *stream, void *const *events);

/* jlm_prime_frames that keeps its states: behind the step of frame f >= n_steps - cap, the live prefix of the state set the step
 * wrote and target[f][0 .. n_live_host[f]) are copied into slot f - (n_steps - cap) of hist [cap][n_rows][H] / words [cap][n_rows]
 * (jlm_cache_store; earlier frames are not stored).  Priming is right-aligned: a row's entries end at slot cap - 1.  Rows past the
 * live prefix of a slot are not written.  1 <= cap; target [n_steps][n_rows] device.  jlm_prime_frames' launches otherwise. */
int jlm_prime_cache_frames(const jlm_decode_model *model_host, const jlm_prime_plan *plan_host, const int *target, void *hist, int *words,
                           int cap, void *stream);

/* ------------------------------------------------------------------------
 * Prediction of an unfinished last word behind a static decode (Decoder.decode_predict; ABI 12, additive).
 * One launch (tail_predict_kernel, csrc/jlm_tail.hip), one workgroup per sentence, on the stream of the jlm_decode_frames whose pools
 * it reads: T / ldt, score, lse, cnt, bp, node of that decode (n_sent, beam, n_frames as its lattice has them; rmax = n_sent * beam).
 * ids [n_ids]: the vocabulary's words sorted by (reading, id) (jlm_amd/readings.py ReadingIndex.ids).  Sentence s has the spans
 * sp_off[s] .. sp_off[s + 1]; span j names the frame sp_frame[j] and the words ids[sp_lo[j] .. sp_hi[j]).  A span whose frame is outside
 * [0, n_frames) or whose words are outside ids[] or empty is skipped.
 * Candidates of a sentence: for every span in order, every word of it in order, every slot k < min(cnt[frame * n_sent + s], beam) of
 * row g = frame * rmax + s * beam + k:  (score[g] + lse[g]) - (double)logit  in f64 (mode 1, self-normalised: score[g] - logit), the
 * logit bit-equal to jlm_edge_logits' for that (row, word) (wordlist_kernel's arithmetic).  Candidate index = position in that order.
 * The n_out (1 .. 64) best by (score, candidate index) ascending -- a NaN score never ranks -- are written at [s * n_out + rank]:
 * out_score, out_row (g), out_word, and the parent's trace as jlm_backtrace writes it: out_nodes[(s * n_out + rank) * stride + d] from
 * node[g] back to the root, out_len.  Ranks beyond the candidate count: (+inf, -1, -1, length 0); a sentence without spans writes
 * only those.  chunk: candidates selected per round with the winners carried so far (LDS holds n_out + chunk + 512 candidates and
 * 16 rows of T whatever the candidate count; 0: 4096); the result does not depend on it.  No atomics; one writer per address.
 * The caller keeps a sentence's candidate count below 2^31.
 * Returns 0, -1 for bad arguments (n_out, beam above JLM_MAX_BEAM, ldt % 4, segments, a null pointer, a chunk whose LDS does not fit),
 * -3, or a hipError_t. */
int jlm_tail_predict(const jlm_segment *segs_host, int n_segs, const float *b2, const float *T, int ldt, int n_sent, int beam,
                     int n_frames, const double *score, const double *lse, const int *cnt, const int *bp, const int *node, int mode,
                     const int *ids, int n_ids, const int *sp_off, const int *sp_frame, const int *sp_lo, const int *sp_hi, int n_out,
                     int chunk, double *out_score, int *out_row, int *out_word, int *out_nodes, int *out_len, int stride, void *stream);

/* ------------------------------------------------------------------------
 * Per-segment candidate lists behind a static decode (Decoder.decode_candidates; ABI 12, additive).
 * Path `rank` of sentence s is the chain of pool rows g_K, bp[g_K], ..., g_0 (the root, bp = -1) from the final row
 * g_K = sent_len[s] * rmax + s * beam + rank (rmax = n_sent * beam); segment k = 1 .. K is the word of g_k.  A row r < n_rows of the call
 * (the rows of a jlm_score_plan) names a sentence, a depth d = k - 1 and a word a: "a in place of the word of segment k".  Its suffix
 * steps j = #{t < n_steps : n_live[t] > r}: the caller sorts rows by j, longest first, as jlm_score_plan wants them.
 * The decode whose pools these are must have completed, or run earlier on the same stream.
 * alt_head_kernel (csrc/jlm_alt.hip), one launch, one workgroup of 256 threads per sentence, writes for every row of the sentence
 *   nll_seq[r] = head + (score[g_K] - score[g_{k+j}]),   head = (score[g_d] + lse[g_d]) - (double)logit(T[g_d], a)   in f64
 *                (mode 1, self-normalised: score[g_d] - logit), the logit bit-equal to jlm_edge_logits' for that (row, word);
 *   prev0[r] = r;  and for j >= 1 rows r of p->h[0] / p->c[0] = the state rows (h, c)[g_d], byte for byte (H 4-byte values each).
 * It replaces the caller's zeroing of nll_seq: jlm_score_frames then adds the j suffix terms.  Rows of the call that no sentence lists
 * are not written.  flags (p->flags, one device int or NULL): |= 1 when an lse read is not finite, |= 2 when a row's word lies in no
 * segment (its nll_seq is NaN), |= 4 when a walk leaves the pool -- a bp outside [-1, n_frames * rmax), a path of n_frames rows or more,
 * sent_len outside [1, n_frames) -- or has fewer segments than a row's depth + 1 + j: such a row gets nll_seq = +inf and prev0 = -1 and
 * nothing is copied for it.  LDS: 16 rows of T, n_frames path entries and n_steps counts, whatever the beam.  No atomics but the flag
 * word's OR; one writer per address. */
typedef struct {
    int n_sent, beam, n_frames, rank;     /* of the decode whose pools these are; 0 <= rank < beam */
    const void *h; const float *c;        /* the decode's state pools (jlm_decode_plan.h / .c) */
    const float *T;                       /* its projection rows, [.., ldt] (jlm_decode_plan.T: untied models, as jlm_tail_predict) */
    const double *score, *lse;            /* jlm_beam_state.score / .lse (lse may be NULL in mode 1) */
    const int *bp;                        /* jlm_beam_state.bp */
    const int *sent_len;                  /* jlm_lattice.sent_len [n_sent] */
    const int *sent_off, *sent_rows;      /* [n_sent + 1], [n_rows] device: the rows of sentence s are sent_rows[sent_off[s] .. sent_off[s + 1]) */
    const int *depth, *alt;               /* [n_rows] device: d = k - 1 and the word a of every row */
    int *prev0;                           /* [n_rows] device, written; must be the score plan's prev0 */
} jlm_alt_plan;

/* -1 before any launch: a null or misaligned pointer (16 bytes: T, the state pools and row sets and the segments' blocks; 8: f64; 4:
 * the rest), beam outside [1, JLM_MAX_BEAM], rank outside [0, beam), ldt % 4, H % 4, mode outside {0, 1}, a->prev0 != p->prev0, a pool of
 * 2^31 rows or more, an LDS request that does not fit.  n_sent == 0 or n_rows == 0: 0, nothing launched.  -3 / a hipError_t as the
 * launchers do.  jlm_alt_head_refuse: the same refusals on their own (0: the launch would be made), no GPU needed. */
int jlm_alt_head_refuse(const jlm_segment *segs_host, int n_segs, const float *b2, int ldt, int H, int mode, const jlm_alt_plan *alt_host,
                        const jlm_score_plan *plan_host);
int jlm_alt_head(const jlm_segment *segs_host, int n_segs, const float *b2, int ldt, int H, int mode, const jlm_alt_plan *alt_host,
                 const jlm_score_plan *plan_host, void *stream);
/* jlm_alt_head, then jlm_score_frames' launches unchanged over plan_host's n_steps steps (none for n_steps == 0), no host
 * synchronisation in between; every refusal of either comes before the first launch.  events as jlm_score_frames'. */
int jlm_alt_frames(const jlm_decode_model *model_host, const jlm_alt_plan *alt_host, const jlm_score_plan *plan_host, void *stream,
                   void *const *events);

/* ------------------------------------------------------------------------
 * Scalar k-means compression of one weight tensor (jlm_amd/compress.py kmeans_compress; the reference's train/comp.py:20-48,
 * scikit-learn KMeans over the flattened weights).  Greedy k-means++ seeding, then Lloyd's iteration, all sums in integers so that
 * the result does not depend on the launch shape or on the order of any accumulation:
 *   mn = min x, mx = max x, e = 36 - (binary exponent of mx - mn as frexp gives it), q_i = min(rint((x_i - mn) 2^e), 2^36 - 1) in f64;
 *   seeding on the histogram of q_i >> 18 (2^18 bins): centre 0 = the bin holding point floor(u N) in bin order; round r >= 1 draws
 *   trials = 2 + floor(ln K) bins with probability ~ count * D^2 (D = bin distance to the nearest chosen centre), target =
 *   floor(u * total) with u = splitmix64(seed, r, t) 2^-64 (sample_rows_kernel's mixer of (r << 32) | (t + 1), all 64 bits), the
 *   first bin whose inclusive prefix exceeds it, and keeps the trial that leaves the smallest total (lowest t on a tie); a round
 *   whose total is 0 repeats the previous centre.  A seeded bin v starts Lloyd at q = (v << 18) + 2^17;
 *   Lloyd on q with centres sorted ascending: i belongs to #{j : c_j + c_(j+1) < 2 q_i}; c_j <- floor((sum + count / 2) / count),
 *   an empty centre stays; it stops after the pass whose largest |shift| <= floor(tol (mx - mn) 2^e), or after max_iter passes;
 *   code_i against the final centres, codebook_j = (float)(mn + c_j 2^-e), ascending.
 * x: n float32 on the device, 16-byte aligned; code: n bytes, 4-byte aligned; codebook: 2^bit float32; scratch: JLM_KMEANS_SCRATCH_BYTES
 * on the device, 16-byte aligned, contents arbitrary.  1 <= n <= JLM_KMEANS_MAX_N (every total fits 64 bits), 1 <= bit <= 8,
 * max_iter >= 1, tol >= 0.  grid: workgroups of the streaming passes (0: four per compute unit); the result does not depend on it.
 * The call WAITS on `stream` (the range, and every JLM_KMEANS_SYNC_EVERY Lloyd passes one flag word, come to the host).
 * info_host[4]: [0] Lloyd passes run [1] 1 for a constant tensor (codebook all mn, codes 0) [2] 1 when x holds a NaN or an infinity
 * (nothing else is written) [3] 0.  ms_host (may be NULL): milliseconds by HIP events of [0] range [1] histogram [2] seeding
 * [3] all Lloyd passes, host waits included [4] final assignment.  Returns 0, -1 for bad arguments, or a hipError_t. */
#define JLM_KMEANS_MAX_N (1ll << 27)
#define JLM_KMEANS_SCRATCH_BYTES ((2u << 20) + 16384u + 65536u)
#define JLM_KMEANS_SYNC_EVERY 8
int jlm_kmeans1d(const float *x, long long n, int bit, uint64_t seed, int max_iter, double tol, unsigned char *code, float *codebook,
                 void *scratch, int grid, int *info_host, float *ms_host, void *stream);

/* ---- training (csrc/jlm_train.hip; jlm_amd/train.py DeviceStepper).  Additive: the ABI version stays 12.
 * Every sum below has one writer and a fixed order: a training step gives the same bits run after run.  All pointers are device
 * pointers to float32 unless said otherwise; every entry launches on `stream` and returns 0, -1 for bad arguments, or a hipError_t.
 *
 * The dropout mask of an [N, width] array (rows in time-major order) is a pure function of (key, row * width + column):
 *   keep <=> (splitmix64 finaliser of key + 0x9E3779B97F4A7C15 (element + 1)) >> 40 < thr,   thr = ceil(keep 2^24),
 * kept values are multiplied by `scale` (1 / keep), the others are zero.  thr = 2^24: everything is kept. */

/* C[M, N] (ldc) (+)= A B (+ bias[N]) with A[m, k] = A[m sam + k sak] and B[k, n] = B[k sbk + n sbn]: the NT, TN (row-contracting) and
 * NN forms by strides.  Per output element an f32 fmaf chain in k order.  accumulate: add to what C holds. */
int jlm_train_gemm(const float *A, long long sam, long long sak, const float *B, long long sbk, long long sbn, float *C, int ldc,
                   int M, int N, int K, int accumulate, const float *bias, void *stream);
/* x[r, :E] = mask (.) emb[ids[r], :E] (ids int32; an id outside [0, V) gives a zero row) */
int jlm_train_embed_rows(const float *emb, int ld_emb, int V, const int *ids, int n_rows, int E, float *x, uint64_t key,
                         unsigned thr, float scale, void *stream);
/* z [B, 4H]: pre-activations i | f | o | g -> activations in place; c = c_prev f + g i; h = tanh(c) o; r = mask (.) h, the mask of rows
 * [row0, row0 + B) of the [N, H] array */
int jlm_train_cell_fwd(float *z, const float *c_prev, float *c, float *h, float *r, int B, int H, long long row0, uint64_t key,
                       unsigned thr, float scale, void *stream);
/* dh = mask (.) dr + dh_next (dh_next may be NULL); dc [B, H] in: the gradient of c from the step after, out: of c_prev; dz [B, 4H] */
int jlm_train_cell_bwd(const float *gates, const float *c, const float *c_prev, const float *dr, const float *dh_next, float *dc,
                       float *dz, int B, int H, long long row0, uint64_t key, unsigned thr, float scale, void *stream);
/* the (max, sum exp) of y[row, :n_cols] merged into run_m / run_s [n_rows] (first: they are overwritten) */
int jlm_train_lse_update(const float *y, int ld, int n_cols, int n_rows, float *run_m, float *run_s, int first, void *stream);
/* y: the logits of words [v0, v0 + n_cols) -> dy = s (p (1 + nw2 lse) - onehot) in place, p = exp(y - lse), lse = run_m + log run_s;
 * tgt_logit[row] = y[row, target[row] - v0] where the target (int32) falls into the chunk.  n_rows <= 65535 */
int jlm_train_dy(float *y, int ld, int n_cols, int v0, int n_rows, const float *run_m, const float *run_s, const int *target,
                 float *tgt_logit, float s, float nw2, void *stream);
/* out[c] (+)= sum over rows of a[r, c], in row order */
int jlm_train_colsum(const float *a, int ld, int n_rows, int n_cols, float *out, int accumulate, void *stream);
/* ce_out[0] (float64) = mean over rows of lse - tgt_logit.  Where the training loss ce + nw mean(lse^2) is not finite in f32 (nw:
 * norm_weight, 0 without self-normalisation) ce_out[0] = +inf and flag[0] = 1 */
int jlm_train_ce(const float *run_m, const float *run_s, const float *tgt_logit, int n_rows, float nw, double *ce_out, int *flag,
                 void *stream);
/* ---- distillation (jlm_amd/distill.py).  Additive: ABI 12.  ys: a student's logits of words [v0, v0 + n_cols),
 * yt: a frozen teacher's logits of the same words, each with its own leading dimension.  run [6, n_rows]: three running (max, sum exp)
 * pairs, rows 0, 1 of ys (L_s), rows 2, 3 of ys inv_tau (A_s), rows 4, 5 of yt inv_tau (A_t); inv_tau = 1 / temperature > 0.
 * Pass 1: the window's pairs merged into run (first: run is overwritten, not read), each logit read once, in granules of 64 words from
 * the window's first as jlm_train_lse_update walks them: at inv_tau == 1 rows 0, 1 are that entry's bits and rows 2, 3 equal them. */
int jlm_distill_lse_update(const float *ys, int ld_s, const float *yt, int ld_t, int n_cols, int n_rows, float inv_tau, float *run,
                           int first, void *stream);
/* Pass 2: ys -> dy = s (c_hard (p - onehot) + nw2 L_s p + c_soft (p^tau - q)) in place, p = exp(ys - L_s), p^tau = exp(ys inv_tau - A_s),
 * q = exp(yt inv_tau - A_t); c_hard = 1 - alpha, c_soft = alpha tau.  tgt_logit as in jlm_train_dy.  kl_row[row] (first: = 0, else +=) the
 * window's sum of q (log q - log p^tau), a q of 0 adding 0: one wave per row, granule sums by butterfly, taken in order. */
int jlm_distill_dy(float *ys, int ld_s, const float *yt, int ld_t, int n_cols, int v0, int n_rows, const float *run, const int *target,
                   float *tgt_logit, float *kl_row, float s, float nw2, float c_hard, float c_soft, float inv_tau, int first, void *stream);
/* kl_out[0] (float64) = mean of kl_row; a value that is not finite gives +inf and flag[0] = 1 */
int jlm_distill_kl(const float *kl_row, int n_rows, double *kl_out, int *flag, void *stream);
/* demb[w - v_lo, e] += sum over the rows r that read word w of mask (.) dx[r, col0 + e], rows in index order, for the words in
 * [v_lo, v_hi) and e < n_cols: the target is that range of words and columns of the [V, width] gradient.  dx [n, ld_dx], the mask that of
 * the [n, width] array; ids_sorted int32 [n] ascending, perm int64 [n] the row of each (a stable sort) */
int jlm_train_scatter_rows(const float *dx, int ld_dx, int col0, int n_cols, int width, const int *ids_sorted, const long long *perm,
                           int n, float *demb, int ld, int v_lo, int v_hi, uint64_t key, unsigned thr, float scale, void *stream);
/* TensorFlow's Adam (beta1 0.9, beta2 0.999, eps 1e-8) over n values, n a multiple of 4, pointers 16-byte aligned; lr_t =
 * lr sqrt(1 - beta2^t) / (1 - beta1^t) from the host.  flag (may be NULL): nothing is updated once flag[0] != 0 */
int jlm_train_adam(float *w, const float *g, float *m, float *v, long long n, float lr_t, const int *flag, void *stream);

/* ---- dynamic evaluation (jlm_amd/dyneval.py).  Additive: ABI 12. */
/* jlm_train_gemm split over the contraction: split s of S = ceil(K / kc) (kc a multiple of 16) runs the same fmaf chain over
 * [s kc, min(K, (s + 1) kc)) and writes its tile to part[s][M][N]; a second launch forms part[0] + part[1] + ... in that order, adds the
 * bias, then C when accumulating, and writes C.  One writer per element, no atomics: the result depends on the operands and kc alone,
 * and with S = 1 it is jlm_train_gemm's bits.  part: part_elems float32 of scratch, -1 when part_elems < S M N. */
int jlm_train_gemm_splitk(const float *A, long long sam, long long sak, const float *B, long long sbk, long long sbn, float *C, int ldc,
                          int M, int N, int K, int accumulate, const float *bias, int kc, float *part, long long part_elems,
                          void *stream);
#define JLM_DYNEVAL_MAX_BLOCKS 4096
/* ms[i] = fmaf(g[i], g[i], ms[i]) over n values, n a multiple of 4, pointers 16-byte aligned.  flag as in jlm_train_adam. */
int jlm_dyneval_sqacc(float *ms, const float *g, long long n, const int *flag, void *stream);
/* rms[i] = sqrtf(ms[i] inv_chunks), and mean_out[0] (float64) = the sum of those f32 values / n_real in a fixed order: per block a partial
 * sum into partial (float64 [JLM_DYNEVAL_MAX_BLOCKS]), then one workgroup adds the partials in index order.  n_real <= n: the number of
 * parameters among the n words (the padding words hold 0). */
int jlm_dyneval_rms(const float *ms, long long n, float inv_chunks, float *rms, long long n_real, double *partial, double *mean_out,
                    void *stream);
/* w = (float)((w - step) + min(lam_scale r, 1) (w0 - w)) evaluated in float64: r = rms[i] and step = lr g / (r + eps), or with rms NULL
 * r = 1 and step = lr g.  One rounding to f32 per element.  n a multiple of 4, pointers 16-byte aligned; flag as in jlm_train_adam. */
int jlm_dyneval_update(float *w, const float *g, const float *w0, const float *rms, long long n, double lr, double lam_scale, double eps,
                       const int *flag, void *stream);

/* ---- fine-tuning the codebooks of a k-means compressed model (jlm_amd/finetune.py).  Additive: ABI 12.
 * A compressed model's weights are w[i] = book[gid[i]] over the flat parameter buffer: book holds every tensor's codebook, tensor t at
 * t K (K = 2^bit); gid[i] = t K + code for a coded element, -1 for the padding between tensors.  The codes never change. */
#define JLM_CODEBOOK_CHUNK 4096
/* w[i] = gid[i] >= 0 ? book[gid[i]] : 0 for i < n (an id >= n_book gives 0 too).  gid int32 [n]; n a multiple of 4, gid and w 16-byte
 * aligned (the accesses to both are 16 bytes wide). */
int jlm_train_expand_codes(const float *book, int n_book, const int *gid, float *w, long long n, void *stream);
/* gbook[j] = the sum of g[i] over the elements i with gid[i] == j, for j < n_groups.  order int32 [n_order]: the offsets of the coded
 * elements sorted by (gid, offset); chunks int32 [n_chunks][3] = (group, begin, length), ascending: every group's run of `order` in
 * pieces of at most JLM_CODEBOOK_CHUNK; partial float64 [n_chunks] scratch.  Two launches: one wave per chunk (lane l adds elements
 * l, l + 64, ... in that order in f64, the lane sums meet in one xor butterfly) -> partial; one lane per group adds its partials in
 * chunk order in f64 and stores the f32 rounding, 0 for a group without chunks.  One writer per sum, a fixed order, no atomics: the
 * bits do not depend on the launch shape.  An offset outside [0, n) or a chunk outside [0, n_order) contributes nothing. */
int jlm_train_codebook_grad(const float *g, long long n, const int *order, long long n_order, const int *chunks, int n_chunks,
                            int n_groups, double *partial, float *gbook, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* JLM_HIP_H */
