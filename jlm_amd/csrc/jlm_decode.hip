// jlm_decode.hip -- the frame loop of a batched decode as one C-ABI call (jlm_decode_frames, include/jlm_hip.h).
// Host code only: it enqueues the launchers of jlm_gemm.hip / jlm_split.hip / jlm_beam.hip in the order
// jlm_amd/engine.py documents, so a batch costs one FFI call instead of ~170.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include "../../include/jlm_hip.h"

namespace {

// fork/join events for the edge-logit side stream.  A wait binds to the record that precedes it at
// enqueue time, so a rotating pool per device is enough; it is sized so that an event is not recorded
// again before the batches that could still be waiting on it (two or three in flight, two events per
// frame) have long been enqueued.
struct EventPool {
    static constexpr int N = 512, MAX_DEV = 16;
    hipEvent_t ev[MAX_DEV][N];
    int next[MAX_DEV] = {0};
    bool ready[MAX_DEV] = {false};
    hipError_t get(hipEvent_t *out) {
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return e;
        if (dev < 0 || dev >= MAX_DEV) return hipErrorInvalidDevice;
        if (!ready[dev]) {
            for (int i = 0; i < N; ++i) {
                e = hipEventCreateWithFlags(&ev[dev][i], hipEventDisableTiming);
                if (e != hipSuccess) return e;
            }
            ready[dev] = true;
        }
        *out = ev[dev][next[dev]];
        next[dev] = (next[dev] + 1) % N;
        return hipSuccess;
    }
};
thread_local EventPool g_events;

#define JLM_TRY(x) do { int rc_ = (x); if (rc_ != 0) return rc_; } while (0)
#define JLM_HIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return (int)e_; } while (0)

}  // namespace

// the refusals of jlm_cache_cell_query / jlm_cache_cell_patch on their own (csrc/jlm_cache_edge.hip)
int jlm_cache_cell_query_refuse(const void *h, int H, int split, float h_scale, const int *g0, const int *cnt, const int *sent_len, int frame,
                                int n_sent, int beam, const void *hist, const int *count, int cap, int n_src, const int *idx, int N,
                                float theta, const float *s, int ld_s, const int *flags);
int jlm_cache_cell_patch_refuse(const float *s, int ld_s, const int *words, const int *count, int cap, int n_src, const int *idx, int N,
                                float lam, const int *cnt, const int *sent_len, int frame, int n_sent, int beam, const int *wl,
                                const int *wl_off, const int *wl_idx, int wl_base, const int *wl_out, const float *edge, const float *part,
                                int ld_part, int n_parts, const int *live_base, const double *lse, const int *flags);
// the refusals of jlm_ngram_cell_patch on their own (csrc/jlm_ngram_edge.hip)
int jlm_ngram_cell_patch_refuse(const void *keys, const float *vals, int log2cap, int max_probe, int order, float lam, const int *g0,
                                const int *cnt, const int *sent_len, int frame, int n_sent, int beam, const int *bp, const int *word,
                                const double *score, const int *root_hist, const int *wl, const int *wl_off, const int *wl_idx, int wl_base,
                                const int *wl_out, const float *edge, const float *part, int ld_part, int n_parts, const int *live_base,
                                const double *lse, const int *flags);
// the refusals of jlm_memory_gather_rows / jlm_memory_cell_patch (csrc/jlm_memory_edge.hip) and jlm_memory_topk (csrc/jlm_memory_topk.hip)
int jlm_memory_gather_rows_refuse(const void *h, int H, long long n_pool_rows, const int *rows, const int *n_dev, int n_rows_max,
                                  const void *out);
int jlm_memory_cell_patch_refuse(const float *s, int ld_s, const int *ret_words, int n_rows, int N, int K, float lam, const int *cnt,
                                 const int *sent_len, int frame, int n_sent, int beam, const int *wl, const int *wl_off, const int *wl_idx,
                                 int wl_base, const int *wl_out, const float *edge, const float *part, int ld_part, int n_parts,
                                 const int *live_base, const double *lse, const int *flags);
int jlm_memory_topk_refuse(const void *keys, const int *key_words, int N, int H, int split, float h_scale, const void *q_rows, int n_rows_max,
                           const int *n_dev, float theta, int K, const float *s, int ld_s, const int *ret_words, const int *ret_idx, int n_rows,
                           const void *workspace, size_t workspace_bytes, const int *flags);

// ABI 11: the model's mixed segments are mx6 rows (FP6 cross-term planes, csrc/jlm_mx6_body.h) when their s8 is 0 -- the hypothesis
// rows are then packed by jlm_pack_t_mixed6; a model mixes the two formats in no launch (jlm_vocab_lse_mixed: -2)
static inline bool jlm_model_mx6(const jlm_decode_model *m) {
    if (!m->mixed_segs || !m->mixed_s8) return false;
    for (int i = 0; i < m->n_segs; ++i)
        if (m->mixed_segs[i].B) return m->mixed_s8[i] == 0.0f;
    return false;
}
#define JLM_PACK_T_MIXED(m) (jlm_model_mx6(m) ? jlm_pack_t_mixed6 : jlm_pack_t_mixed)

// ---- the full-vocabulary normaliser (kind 0) of one step's rows, shared by the frame loop and the scoring loop (jlm_score_frames).
// Two halves: full_lse_pack right behind the T projection (the packed rows of the mixed segments, if the model has them), and
// full_lse_run after it (the decode enqueues its edge logits in between), which leaves the (max, sum exp) slices in `part`.
// a segment with k > 256 (untied models: k = H) is outside the rows-stationary normalisers: one tile GEMM per segment
// with a per-tile log-sum-exp epilogue (jlm_vocab_lse_partials), its slices folded by the consumer of the slices
static bool full_lse_tile_form(const jlm_decode_model *m) {
    if (m->self_norm) return false;
    for (int i = 0; i < m->n_segs; ++i)
        if (m->segs[i].k > 256) return true;
    return false;
}

struct FullLse {
    bool tile_form = false, hybrid = false, all_mixed = false;
};

// segments of the full-vocabulary normaliser on mixed rows: the step's live rows are packed once, here, behind T
// (round 5: an untied model at H = 512 -- T is the state's f32 copy, one segment of k = 512 -- runs jlm_vocab_lse_mixed's wide
//  one-row-set form instead of the tile GEMM below when its vocabulary matrix exists as mixed rows)
static int full_lse_pack(const jlm_decode_model *m, const float *T, const int *rows, int bound, const int *ndev, void *Tm, int ld_tm,
                         bool skip_pack, FullLse &fl, void *stream) {
    fl = FullLse();
    fl.tile_form = full_lse_tile_form(m);
    if (m->self_norm) return 0;
    const bool untied_mixed = fl.tile_form && m->untied && m->n_segs == 1 && m->mixed_segs && m->mixed_segs[0].B && Tm;
    if ((!fl.tile_form && m->mixed_segs && m->split_segs && Tm) || untied_mixed) {
        jlm_segment only[JLM_MAX_SEGMENTS];
        float only_ts[JLM_MAX_SEGMENTS];
        int n_only = 0;
        for (int i = 0; i < m->n_segs; ++i)
            if (m->mixed_segs[i].B) { only[n_only] = m->mixed_segs[i]; only_ts[n_only++] = m->mixed_t_scale[i]; }
        if (n_only) {
            if (jlm_mixed_t_stride(only, n_only) != ld_tm) return -1;
            if (!skip_pack) JLM_TRY(JLM_PACK_T_MIXED(m)(only, only_ts, n_only, T, m->ldt, rows, bound, ndev, Tm, ld_tm, stream));
            fl.hybrid = true;
            fl.all_mixed = n_only == m->n_segs;
            // (ABI 10) a segment whose head stays on split rows: the launch over both formats
            if (fl.all_mixed && m->mixed_head_split && m->split_segs)
                for (int i = 0; i < m->n_segs; ++i)
                    if (m->mixed_head_split[i] > 0) fl.all_mixed = false;
        }
    }
    return 0;
}

// -> *n_parts slices [n][ld_part] (indexed by compact row).  bound: static bound of the live rows (the column count follows it);
// tile_rows: the row bound of the tile form's launches; h: the state rows the step wrote (untied split-row models read them).
static int full_lse_run(const jlm_decode_model *m, const FullLse &fl, const float *T, const void *h, const void *Tm, int ld_tm,
                        const int *rows, int ld_part, int bound, int tile_rows, const int *ndev, float *part, int max_parts,
                        int lse_cu_share_pct, int *n_parts_out, void *stream) {
    *n_parts_out = 0;
    if (fl.tile_form && !fl.all_mixed) {
        int n_parts = 0;
        for (int i = 0; i < m->n_segs; ++i) {
            const jlm_segment &sg = m->segs[i];
            // capacity is checked BEFORE the launch that would write the slices (one per 128-word tile)
            if (n_parts + (sg.v_end - sg.v_start + 127) / 128 > max_parts) return -1;
            int r = (m->untied && m->untied_split && m->split_lstm)
                        ? jlm_vocab_lse_partials_split(m->untied_split, m->H, sg.v_end - sg.v_start, m->H, h, m->H, rows,
                                                       m->b2 + sg.v_start, m->untied_descale, part, ld_part, n_parts,
                                                       tile_rows, ndev, stream)
                        : jlm_vocab_lse_partials(sg.B, sg.ldb, sg.v_end - sg.v_start, sg.k, T + sg.t_off, m->ldt, rows,
                                                 m->b2 + sg.v_start, part, ld_part, n_parts, tile_rows, ndev, stream);
            if (r < 0) return r;
            n_parts += r;
        }
        if (n_parts > max_parts) return -1;
        *n_parts_out = n_parts;
        return 0;
    }
    // the share of the chip this batch's normaliser takes: its range count is capped so that ranges x row tiles
    // (one 8-wave workgroup per CU each) fill that share; the launcher rounds down to a multiple of 8 ranges
    int cap = max_parts;
    if (lse_cu_share_pct > 0 && lse_cu_share_pct < 100) {
        const int n_ptiles = (bound + 255) / 256;
        int c = 256 * lse_cu_share_pct / 100 / n_ptiles;
        if (c < 1) c = 1;
        c += m->n_segs - 1;            // slices = columns + the segment boundaries columns straddle
        if (c < cap) cap = c;
    }
    int r = -2;
    if (fl.all_mixed)      // every segment on mixed rows (lse_fixed_ref: without a running maximum where the kernel has such a form)
        r = (m->lse_fixed_ref ? jlm_vocab_lse_mixed_fr : jlm_vocab_lse_mixed)(m->mixed_segs, m->mixed_descale, m->mixed_s8, m->mixed_bias2,
                                                                             m->n_segs, Tm, ld_tm, part, ld_part, cap, bound, ndev, stream);
    else if (fl.hybrid)    // -2: a shape the hybrid kernel does not host -- the split rows of every segment exist
        r = jlm_vocab_lse_hybrid(m->split_segs, m->split_t_scale, m->split_descale, m->split_bias_col, m->mixed_segs,
                                 m->mixed_descale, m->mixed_s8, m->mixed_head_split, m->n_segs, m->b2, T, m->ldt, Tm,
                                 ld_tm, rows, part, ld_part, cap, bound, ndev, stream);
    if (r == -2)
        r = m->split_segs
                ? jlm_vocab_lse_split(m->split_segs, m->split_t_scale, m->split_descale, m->split_bias_col,
                                      m->n_segs, m->b2, T, m->ldt, rows, part, ld_part, cap, bound,
                                      ndev, stream)
                : jlm_vocab_lse_stationary(m->segs, m->n_segs, m->b2, T, m->ldt, rows, part, ld_part,
                                           max_parts, bound, ndev, stream);
    if (r < 0) return r;
    *n_parts_out = r;
    return 0;
}

extern "C" int jlm_decode_frames(const jlm_decode_model *m, const jlm_decode_plan *p, const jlm_lattice *lat,
                                 const jlm_beam_state *st_in, void *stream, void *side_stream, void *const *events) {
    const int B = lat->n_sent, beam = lat->beam, F = lat->n_frames;
    const int rmax = B * beam;
    const bool dynamic = p->kind == 2, select = p->kind == 1, full = p->kind == 0;
    const int mode = m->self_norm ? 1 : (dynamic ? 2 : 0);
    jlm_beam_state st = *st_in;
    hipStream_t main_s = (hipStream_t)stream, side_s = events ? nullptr : (hipStream_t)side_stream;
    // events != NULL: JLM_EVENTS_PER_FRAME timing events per frame, recorded on `stream` (no side stream then, so that
    // every bracket holds exactly the kernels it names)
    auto stamp = [&](int f, int i) -> int {
        if (!events) return 0;
        return (int)hipEventRecord((hipEvent_t)events[(size_t)f * JLM_EVENTS_PER_FRAME + i], main_s);
    };
    hipEvent_t join = nullptr;
    int pending_parts = 0;
    // The continuous cache (jlm_decode_plan.cache, kind 0): behind the normaliser and the edge logits of every frame, the cache scores
    // of the frame's hypotheses (jlm_cache_cell_query) and the rewrite of the edge logits leaving it (jlm_cache_cell_patch), which also
    // folds the frame's normaliser slices -- the next beam step then runs unfused.  The edge logits stay on the main stream.  Every
    // refusal comes here, before the first launch.
    const jlm_decode_cache *cc = p->cache;
    const int split = m->split_lstm ? 1 : 0;
    if (cc) {
        if (!full || !st.live_base || (!m->self_norm && (!p->part || p->max_parts < 1))) return -1;
        JLM_TRY(jlm_cache_cell_query_refuse(p->h, m->H, split, m->h_scale, p->g0, st.cnt, lat->sent_len, 0, B, beam, cc->hist, cc->count,
                                            cc->cap, cc->n_src, cc->idx, cc->N, cc->theta, cc->s, cc->ld_s, st.flags));
        JLM_TRY(jlm_cache_cell_patch_refuse(cc->s, cc->ld_s, cc->words, cc->count, cc->cap, cc->n_src, cc->idx, cc->N, cc->lam, st.cnt,
                                            lat->sent_len, 0, B, beam, p->sg_word, p->sg_off, p->sidx, 0, p->sg_node, p->edge,
                                            m->self_norm ? nullptr : p->part, rmax, 1, st.live_base, st.lse, st.flags));
        side_s = nullptr;
    }
    // A back-off n-gram model (jlm_decode_plan.ngram, kind 0): behind the normaliser and the edge logits of every frame, the rewrite of
    // the edge logits leaving it (jlm_ngram_cell_patch), which folds the frame's normaliser slices as the cache's patch does.  Not beside
    // the cache: a three-way mixture is not defined.  Every refusal comes here, before the first launch.
    const jlm_decode_ngram *ng = p->ngram;
    if (ng) {
        if (cc || !full || !st.live_base || (!m->self_norm && (!p->part || p->max_parts < 1))) return -1;
        JLM_TRY(jlm_ngram_cell_patch_refuse(ng->keys, ng->vals, ng->log2cap, ng->max_probe, ng->order, ng->lam, p->g0, st.cnt, lat->sent_len,
                                            0, B, beam, st.bp, st.word, st.score, ng->root_hist, p->sg_word, p->sg_off, p->sidx, 0,
                                            p->sg_node, p->edge, m->self_norm ? nullptr : p->part, rmax, 1, st.live_base, st.lse, st.flags));
        side_s = nullptr;
    }
    // A memory of (hidden state, next word) pairs (jlm_decode_plan.memory, kind 0): behind the normaliser and the edge logits of every
    // frame, the frame's live rows gathered into contiguous query rows (jlm_memory_gather_rows), their K nearest entries
    // (jlm_memory_topk) and the rewrite of the edge logits leaving the frame (jlm_memory_cell_patch), which folds the frame's normaliser
    // slices as the cache's patch does.  Not beside the cache or the n-gram model: a three-way mixture is not defined.  Every refusal
    // comes here, before the first launch.
    const jlm_decode_memory *mem = p->memory;
    const long long pool_rows = (long long)F * rmax;
    if (mem) {
        if (cc || ng || !full || !st.live_base || (!m->self_norm && (!p->part || p->max_parts < 1)) || rmax > 65535) return -1;
        JLM_TRY(jlm_memory_gather_rows_refuse(p->h, m->H, pool_rows, st.live, st.n_live, rmax, mem->q_rows));
        JLM_TRY(jlm_memory_topk_refuse(mem->keys, mem->key_words, mem->N, m->H, split, m->h_scale, mem->q_rows, rmax, st.n_live, mem->theta,
                                       mem->K, mem->s, mem->ld_s, mem->ret_words, nullptr, rmax, mem->workspace, mem->workspace_bytes,
                                       mem->flags));
        JLM_TRY(jlm_memory_cell_patch_refuse(mem->s, mem->ld_s, mem->ret_words, rmax, mem->N, mem->K, mem->lam, st.cnt, lat->sent_len, 0, B,
                                             beam, p->sg_word, p->sg_off, p->sidx, 0, p->sg_node, p->edge, m->self_norm ? nullptr : p->part,
                                             rmax, 1, st.live_base, st.lse, st.flags));
        side_s = nullptr;
    }

    // word-list normaliser: the kernel jlm_wordlist_lse_form names (split rows for lists of 128 .. 4064 words)
    auto wl_lse = [&](const int *g0, const int *cidx, const int *words, const int *off, const int *idx, int base, int merge,
                      int n_groups, int max_words) -> int {
        if (jlm_wordlist_lse_form(m->segs, m->n_segs, m->split_segs, 0, m->ldt, beam, max_words) == JLM_WL_SPLIT)
            return jlm_wordlist_lse_split(m->split_segs, m->split_t_scale[0], m->split_descale[0], m->b2, p->T, m->ldt, g0,
                                          st.cnt, cidx, words, off, idx, base, max_words, p->run_max, p->run_sum, st.lse,
                                          merge, beam, n_groups, stream);
        return jlm_wordlist_lse(m->segs, m->n_segs, m->b2, p->T, m->ldt, g0, st.cnt, cidx, words, off, idx, base,
                                p->run_max, p->run_sum, st.lse, merge, beam, n_groups, stream);
    };
    // reference-compatibility mode of the incremental decoder on segmented models (jlm_decode_plan.di_wwords)
    const bool perm = dynamic && p->di_wwords && p->sg_wword;

#ifdef JLM_PROBE_SKIP
    // measurement builds only (tools/probes/skip_kernel.sh): JLM_SKIP=<bits> leaves launches out -- 1 edge logits, 2 T projection,
    // 4 LSTM step, 8 beam step, 16 vocabulary kernel, 32 packing of the T rows.  Results are wrong; the step time says what is on the critical path.
    // JLM_SKIP_AFTER=n: the first n frame loops run complete, so that the buffers a skipped kernel would have written hold
    // data of the usual kind (zeros in the operands of the matrix kernels draw less power: the clock rises and the probe lies)
    static const int skip_bits = [] { const char *e = getenv("JLM_SKIP"); return e ? atoi(e) : 0; }();
    static const int skip_after = [] { const char *e = getenv("JLM_SKIP_AFTER"); return e ? atoi(e) : 0; }();
    static int n_loops = 0;
    const int skip = (n_loops++ >= skip_after) ? skip_bits : 0;
#define JLM_SKIPPED(bit) (skip & (bit))
#else
#define JLM_SKIPPED(bit) 0
#endif
    // The fused frame tail (jlm_pack_edge_mx6, csrc/jlm_frame_tail.hip): the full-vocabulary decode of a model whose every segment is on
    // mx6 rows packs the live rows inside the edge-logit launch -- one launch and one pass over T less per frame.  JLM_FUSE_TAIL=0 keeps
    // the two launches (A/B runs); so does a probe build that leaves one of the two out, so that the probe means what it says.
    jlm_segment tail_segs[JLM_MAX_SEGMENTS];
    float tail_ts[JLM_MAX_SEGMENTS];
    bool fuse_tail = false;
    if (full && !m->self_norm && !full_lse_tile_form(m) && jlm_model_mx6(m) && m->split_segs && p->Tm && st.live_base && !JLM_SKIPPED(1 | 32)) {
        static const bool on = [] { const char *e = getenv("JLM_FUSE_TAIL"); return !e || atoi(e) != 0; }();
        fuse_tail = on;
        for (int i = 0; i < m->n_segs && fuse_tail; ++i) {
            if (!m->mixed_segs[i].B || m->mixed_s8[i] != 0.0f) {
                fuse_tail = false;
                break;
            }
            tail_segs[i] = m->mixed_segs[i];
            tail_ts[i] = m->mixed_t_scale[i];
        }
        // (no groups: the launcher only says whether it hosts the shape -- beam <= 16, k <= 256, 32 KB of LDS)
        if (fuse_tail && jlm_pack_edge_mx6(m->segs, m->n_segs, m->b2, tail_segs, tail_ts, m->n_segs, p->T, m->ldt, p->g0, st.cnt, p->cidx, p->sg_word,
                                           p->sg_off, p->sidx, 0, p->sg_node, p->edge, beam, 0, lat->sent_len, st.live_base, 0, p->Tm, p->ld_tm,
                                           stream) != 0)
            fuse_tail = false;
    }
    for (int f = 0; f < F; ++f) {
        if (join) {
            JLM_HIP(hipStreamWaitEvent(main_s, join, 0));
            join = nullptr;
        }
        JLM_TRY(stamp(f, 0));
        if (dynamic && !m->self_norm && f >= 2) {
            if (jlm_wordlist_merge_form(m->segs, m->n_segs, m->split_segs, m->ldt, beam, p->dd_max) == JLM_WL_MERGE_SPLIT)
                JLM_TRY(jlm_wordlist_merge_split(m->split_segs, m->split_t_scale[0], m->split_descale[0], m->b2, p->T, m->ldt,
                                                 st.cnt, B, beam, f - 1, p->dd_words, p->dd_off, f * B, p->dd_max, p->run_max,
                                                 p->run_sum, st.lse, stream));
            else
                JLM_TRY(wl_lse(p->g0, p->cidx, p->dd_words, p->dd_off, p->sidx, f * B, 1, (f - 1) * B, p->dd_max));
        }
        JLM_TRY(stamp(f, 1));
        st.lse_part = pending_parts ? p->part : nullptr;
        st.ld_part = rmax;
        st.n_parts = pending_parts;
        if (!JLM_SKIPPED(8)) JLM_TRY(jlm_beam_step(lat, &st, f, mode, p->max_cands, stream));
        JLM_TRY(stamp(f, 2));
        pending_parts = 0;
        if (f == F - 1) break;
        const int *rows = st.live + (size_t)f * rmax;
        const int *ndev = st.n_live + f;
        // frame 0 with a left context: the root rows continue the primed states jlm_seed_context left behind the pool
        const bool seeded = f == 0 && p->ctx_prev && p->ctx_word;
        const int *step_prev = seeded ? p->ctx_prev : st.bp, *step_word = seeded ? p->ctx_word : st.word;
        if (JLM_SKIPPED(4)) {
        } else if (m->split_lstm && m->wt8)
            JLM_TRY(jlm_lstm_step_xg(p->h, p->c, m->H, p->h, p->c, rows, step_prev, step_word, m->wt8, m->xgate8, m->H,
                                     m->gate_descale, m->h_scale, m->untied ? p->T : nullptr, rmax, ndev, stream));
        else if (m->split_lstm)
            return -2;              // (a split-row model always carries wt8 / xgate8: DeviceModel builds them together)
        else
            JLM_TRY(jlm_lstm_step((const float *)p->h, p->c, m->H, (float *)p->h, p->c, rows, step_prev, step_word, m->emb,
                                  m->ld_emb, m->wt, m->gate_bias, m->kpad, m->H, m->E, rmax, ndev, stream));
        JLM_TRY(stamp(f, 3));
        if (!m->untied && !JLM_SKIPPED(2)) {
            if (m->split_lstm)
                JLM_TRY(jlm_gemm_nt_split(p->h, m->H, rows, m->pmt_split, m->H, nullptr, p->T, m->ldt, rows, nullptr,
                                          m->t_descale, rmax, m->n_t, m->H, ndev, stream));
            else
                JLM_TRY(jlm_gemm_nt((const float *)p->h, m->H, rows, m->pmt, m->H, nullptr, p->T, m->ldt, rows, nullptr, rmax,
                                    m->n_t, m->H, ndev, stream));
        }
        // the packed rows of the normaliser's mixed segments, behind T (the normaliser itself runs after the edge logits: full_lse_run);
        // slices of a tile-form normaliser (k > 256) are folded by the next frame's beam step like the others
        FullLse fl;
        if (full) JLM_TRY(full_lse_pack(m, p->T, rows, f == 0 ? B : rmax, ndev, p->Tm, p->ld_tm, JLM_SKIPPED(32) || fuse_tail, fl, stream));
        const int cell = f * B;
        void *est = stream;
        if (fuse_tail) {       // packing and edge logits in one launch behind T, on the main stream: nothing is left to run beside the normaliser
            JLM_TRY(jlm_pack_edge_mx6(m->segs, m->n_segs, m->b2, tail_segs, tail_ts, m->n_segs, p->T, m->ldt, p->g0 + cell, st.cnt, p->cidx + cell,
                                      p->sg_word, p->sg_off, p->sidx, cell, p->sg_node, p->edge, beam, B, lat->sent_len, st.live_base + cell, f,
                                      p->Tm, p->ld_tm, stream));
        } else if (side_s) {   // the edge logits need only T: they run beside the normaliser
            hipEvent_t fork;
            JLM_HIP(g_events.get(&fork));
            JLM_HIP(hipEventRecord(fork, main_s));
            JLM_HIP(hipStreamWaitEvent(side_s, fork, 0));
            est = side_stream;
        }
        if (!fuse_tail && !JLM_SKIPPED(1)) JLM_TRY(jlm_edge_logits_perm(m->segs, m->n_segs, m->b2, p->T, m->ldt, p->g0 + cell, st.cnt, p->cidx + cell, p->sg_word,
                                     perm ? p->sg_wword : nullptr, p->sg_off, p->sidx, cell, p->sg_node, p->edge, beam, B, est));
        if (side_s && !fuse_tail) {
            JLM_HIP(g_events.get(&join));
            JLM_HIP(hipEventRecord(join, side_s));
        }
        JLM_TRY(stamp(f, 4));
        if (!m->self_norm && !JLM_SKIPPED(16)) {
            if (perm)
                JLM_TRY(jlm_wordlist_lse_perm(m->segs, m->n_segs, m->b2, p->T, m->ldt, p->g0 + cell, st.cnt, p->cidx + cell,
                                              p->di_words, p->di_wwords, p->di_off, p->di_idx, 2 * cell, p->run_max, p->run_sum,
                                              st.lse, 0, beam, B, stream));
            else if (dynamic)
                JLM_TRY(wl_lse(p->g0 + cell, p->cidx + cell, p->di_words, p->di_off, p->di_idx, 2 * cell, 0, B, p->di_max));
            else if (select)
                JLM_TRY(wl_lse(p->g0 + cell, p->cidx + cell, p->vs_words, p->vs_off, p->sidx, 0, 0, B, p->vs_max));
            else      // frame 0 has one row per sentence: the bound lets the kernel cut the vocabulary into more ranges
                JLM_TRY(full_lse_run(m, fl, p->T, p->h, p->Tm, p->ld_tm, rows, rmax, f == 0 ? B : rmax, rmax, ndev, p->part, p->max_parts,
                                     p->lse_cu_share_pct, &pending_parts, stream));
        }
        JLM_TRY(stamp(f, 5));
        if (cc) {
            JLM_TRY(jlm_cache_cell_query(p->h, m->H, split, m->h_scale, p->g0 + cell, st.cnt + cell, lat->sent_len, f, B, beam, cc->hist,
                                         cc->count, cc->cap, cc->n_src, cc->idx, cc->N, cc->theta, cc->s, cc->ld_s, st.flags, stream));
            JLM_TRY(jlm_cache_cell_patch(cc->s, cc->ld_s, cc->words, cc->count, cc->cap, cc->n_src, cc->idx, cc->N, cc->lam, st.cnt + cell,
                                         lat->sent_len, f, B, beam, p->sg_word, p->sg_off, p->sidx, cell, p->sg_node, p->edge,
                                         pending_parts ? p->part : nullptr, rmax, pending_parts, st.live_base + cell,
                                         st.lse + (size_t)f * rmax, st.flags, stream));
            pending_parts = 0;             // folded: the next beam step reads lse
        }
        if (ng) {
            JLM_TRY(jlm_ngram_cell_patch(ng->keys, ng->vals, ng->log2cap, ng->max_probe, ng->order, ng->lam, p->g0 + cell, st.cnt + cell,
                                         lat->sent_len, f, B, beam, st.bp, st.word, st.score, ng->root_hist, p->sg_word, p->sg_off, p->sidx,
                                         cell, p->sg_node, p->edge, pending_parts ? p->part : nullptr, rmax, pending_parts,
                                         st.live_base + cell, st.lse + (size_t)f * rmax, st.flags, stream));
            pending_parts = 0;             // folded: the next beam step reads lse
        }
        if (mem) {
            const int bound = f == 0 ? B : rmax;
            JLM_TRY(jlm_memory_gather_rows(p->h, m->H, pool_rows, rows, ndev, bound, mem->q_rows, stream));
            JLM_TRY(jlm_memory_topk(mem->keys, mem->key_words, mem->N, m->H, split, m->h_scale, mem->q_rows, bound, ndev, mem->theta, mem->K,
                                    mem->s, mem->ld_s, mem->ret_words, nullptr, rmax, mem->workspace, mem->workspace_bytes, mem->flags,
                                    stream));
            JLM_TRY(jlm_memory_cell_patch(mem->s, mem->ld_s, mem->ret_words, rmax, mem->N, mem->K, mem->lam, st.cnt + cell, lat->sent_len, f, B,
                                          beam, p->sg_word, p->sg_off, p->sidx, cell, p->sg_node, p->edge, pending_parts ? p->part : nullptr,
                                          rmax, pending_parts, st.live_base + cell, st.lse + (size_t)f * rmax, st.flags, stream));
            pending_parts = 0;             // folded: the next beam step reads lse
        }
    }
    if (join) JLM_HIP(hipStreamWaitEvent(main_s, join, 0));
    return jlm_backtrace(lat, &st, p->out_nodes, p->out_len, p->out_score, p->stride, stream);
}

// ABI 8: the full-vocabulary normaliser of a few PROBE rows, in the form asked for -- what DeviceModel's load-time calibration
// of the mixed rows runs (jlm_amd/model.py _calibrate_mixed): `steps` LSTM steps from the zero state over given words, the T
// projection of the last step's rows, then jlm_vocab_lse_split (form 0) or exactly what jlm_decode_frames launches for a model
// with mixed rows (form 1: jlm_pack_t_mixed + jlm_vocab_lse_mixed / _hybrid).  Row g = t * rows + r is hypothesis r after t
// steps; rowlist[g] = g, prev[g] = g - rows (< 0 for block 1: zero state), word[g] = the word consumed by step t.
extern "C" int jlm_lse_probe(const jlm_decode_model *m, const int *rowlist, const int *prev, const int *word, int steps, int rows,
                             void *h, float *c, float *T, void *Tm, int ld_tm, int form, float *part, int max_parts, void *stream) {
    if (steps < 1 || rows < 1 || !m->split_lstm || !m->wt8 || m->self_norm) return -2;
    if (m->untied) {
        // an untied model (round 5): T is the f32 copy of the state the step writes beside its split rows; form 0 = the tile GEMM on
        // split rows (jlm_vocab_lse_partials_split), form 1 = the mixed rows of the vocabulary matrix (k = 512: the wide kernel)
        if (!m->untied_split || m->n_segs != 1) return -2;
        for (int t = 1; t <= steps; ++t)
            JLM_TRY(jlm_lstm_step_xg(h, c, m->H, h, c, rowlist + (size_t)t * rows, prev, word, m->wt8, m->xgate8, m->H, m->gate_descale,
                                     m->h_scale, T, rows, nullptr, stream));
        const int *rl = rowlist + (size_t)steps * rows;
        const jlm_segment &sg = m->segs[0];
        if (form == 0) {
            if ((sg.v_end - sg.v_start + 127) / 128 > max_parts) return -1;
            return jlm_vocab_lse_partials_split(m->untied_split, m->H, sg.v_end - sg.v_start, m->H, h, m->H, rl, m->b2 + sg.v_start,
                                                m->untied_descale, part, rows, 0, rows, nullptr, stream);
        }
        if (!m->mixed_segs || !m->mixed_segs[0].B || !Tm) return -2;
        if (jlm_mixed_t_stride(m->mixed_segs, 1) != ld_tm) return -1;
        JLM_TRY(JLM_PACK_T_MIXED(m)(m->mixed_segs, m->mixed_t_scale, 1, T, m->ldt, rl, rows, nullptr, Tm, ld_tm, stream));
        return (m->lse_fixed_ref ? jlm_vocab_lse_mixed_fr : jlm_vocab_lse_mixed)(m->mixed_segs, m->mixed_descale, m->mixed_s8, m->mixed_bias2, 1, Tm,
                                                                                 ld_tm, part, rows, max_parts, rows, nullptr, stream);
    }
    if (!m->split_segs || !m->pmt_split) return -2;
    for (int t = 1; t <= steps; ++t)
        JLM_TRY(jlm_lstm_step_xg(h, c, m->H, h, c, rowlist + (size_t)t * rows, prev, word, m->wt8, m->xgate8, m->H, m->gate_descale,
                                 m->h_scale, nullptr, rows, nullptr, stream));
    const int *rl = rowlist + (size_t)steps * rows;
    JLM_TRY(jlm_gemm_nt_split(h, m->H, rl, m->pmt_split, m->H, nullptr, T, m->ldt, rl, nullptr, m->t_descale, rows, m->n_t, m->H,
                              nullptr, stream));
    if (form == 0)
        return jlm_vocab_lse_split(m->split_segs, m->split_t_scale, m->split_descale, m->split_bias_col, m->n_segs, m->b2, T, m->ldt, rl,
                                   part, rows, max_parts, rows, nullptr, stream);
    if (!m->mixed_segs || !Tm) return -2;
    jlm_segment only[JLM_MAX_SEGMENTS];
    float only_ts[JLM_MAX_SEGMENTS];
    int n_only = 0;
    for (int i = 0; i < m->n_segs; ++i)
        if (m->mixed_segs[i].B) { only[n_only] = m->mixed_segs[i]; only_ts[n_only++] = m->mixed_t_scale[i]; }
    if (!n_only || jlm_mixed_t_stride(only, n_only) != ld_tm) return -1;
    JLM_TRY(JLM_PACK_T_MIXED(m)(only, only_ts, n_only, T, m->ldt, rl, rows, nullptr, Tm, ld_tm, stream));
    bool cut = false;
    if (m->mixed_head_split)
        for (int i = 0; i < m->n_segs; ++i)
            if (m->mixed_segs[i].B && m->mixed_head_split[i] > 0) cut = true;
    if (n_only == m->n_segs && !cut)       // (the form the decode launches: without a running maximum when the model says so)
        return (m->lse_fixed_ref ? jlm_vocab_lse_mixed_fr : jlm_vocab_lse_mixed)(m->mixed_segs, m->mixed_descale, m->mixed_s8, m->mixed_bias2,
                                                                                 m->n_segs, Tm, ld_tm, part, rows, max_parts, rows, nullptr, stream);
    return jlm_vocab_lse_hybrid(m->split_segs, m->split_t_scale, m->split_descale, m->split_bias_col, m->mixed_segs, m->mixed_descale,
                                m->mixed_s8, m->mixed_head_split, m->n_segs, m->b2, T, m->ldt, Tm, ld_tm, rl, part, rows, max_parts, rows,
                                nullptr, stream);
}

// The LSTM step and the T projection of a row set's live prefix r < *ndev (bound: its static bound; g = rows[r] = r) -- the launches of
// one step of jlm_score_frames and jlm_generate_frames.  f32_copy: the plain f32 copy of the new state an untied split-row model's
// vocabulary GEMMs read (its T); T: the projection's destination (not written on untied models: T is the state there).
static int rows_lstm_step(const jlm_decode_model *m, const void *h_in, const float *c_in, void *h_out, float *c_out, const int *rows,
                          const int *prev, const int *word, float *f32_copy, int bound, const int *ndev, void *stream) {
    if (m->split_lstm)
        return jlm_lstm_step_xg(h_in, c_in, m->H, h_out, c_out, rows, prev, word, m->wt8, m->xgate8, m->H, m->gate_descale, m->h_scale,
                                m->untied ? f32_copy : nullptr, bound, ndev, stream);
    return jlm_lstm_step((const float *)h_in, c_in, m->H, (float *)h_out, c_out, rows, prev, word, m->emb, m->ld_emb, m->wt,
                         m->gate_bias, m->kpad, m->H, m->E, bound, ndev, stream);
}

static int rows_t_projection(const jlm_decode_model *m, const void *h_out, const int *rows, float *T, int bound, const int *ndev,
                             void *stream) {
    if (m->untied) return 0;
    if (m->split_lstm)
        return jlm_gemm_nt_split(h_out, m->H, rows, m->pmt_split, m->H, nullptr, T, m->ldt, rows, nullptr, m->t_descale, bound, m->n_t,
                                 m->H, ndev, stream);
    return jlm_gemm_nt((const float *)h_out, m->H, rows, m->pmt, m->H, nullptr, T, m->ldt, rows, nullptr, bound, m->n_t, m->H, ndev,
                       stream);
}

// The full-vocabulary logits of rows 0 .. n_rows - 1 of T: one jlm_gemm_nt per segment into columns v_start .. v_end of `logits`
// (+ b2) -- the logit GEMMs of jlm_generate_frames and jlm_complete_frames.
static int rows_logits(const jlm_decode_model *m, const float *T, float *logits, int ld_logits, int n_rows, void *stream) {
    for (int i = 0; i < m->n_segs; ++i) {
        const jlm_segment &sg = m->segs[i];
        JLM_TRY(jlm_gemm_nt(T + sg.t_off, m->ldt, nullptr, sg.B, sg.ldb, nullptr, logits + sg.v_start, ld_logits, nullptr,
                            m->b2 + sg.v_start, n_rows, sg.v_end - sg.v_start, sg.k, nullptr, stream));
    }
    return 0;
}

// The frame loops over row sets.  An untied f32 model's T is the state row set the step wrote; every other model has its own T rows
// (an untied split-row model: the f32 copy the step writes beside the split rows).
static bool t_is_state(const jlm_decode_model *m) { return m->untied && !m->split_lstm; }

// -2: a split-row model without wt8 / xgate8 (DeviceModel builds them together); -1: no T rows where T is not the state
static int rows_refuse(const jlm_decode_model *m, const float *T) { return m->split_lstm && !m->wt8 ? -2 : !T && !t_is_state(m) ? -1 : 0; }
// -1: a row of logits that is no multiple of 4 floats or shorter than V rounded up to one
static int logits_refuse(int ld_logits, int V) { return ld_logits % 4 != 0 || ld_logits < ((V + 3) & ~3) ? -1 : 0; }

// event i of frame f, per_frame events a frame (none when the call is untimed: events NULL)
struct Stamps {
    void *const *events;
    int per_frame;
    void *stream;
    int operator()(int f, int i) const {
        return events ? (int)hipEventRecord((hipEvent_t)events[(size_t)f * per_frame + i], (hipStream_t)stream) : 0;
    }
};

// frame f reads state set f % 2 and writes the other; T: where the T projection writes (the written set when t_is_state)
struct PingPong {
    void *h_in, *h_out;
    float *c_in, *c_out, *T;
    PingPong(const jlm_decode_model *m, void *const h[2], float *const c[2], float *T_rows, int f)
        : h_in(h[f & 1]), h_out(h[(f + 1) & 1]), c_in(c[f & 1]), c_out(c[(f + 1) & 1]), T(t_is_state(m) ? (float *)h_out : T_rows) {}
};

// Stamp 0, the LSTM step and stamp 1 of frame f of jlm_generate_frames / jlm_complete_frames.  A prompt frame (f < n_prompt) steps
// the live prefix n_live_host[f] of the right-aligned prompts, from row f of prompt / prev (stride: the rows of a prompt frame --
// n_rows in generate, n_prompts in complete); every later frame steps all n_rows rows from word / prev_rows.
template <class Plan>
static int frame_lstm_step(const jlm_decode_model *m, const Plan *p, const PingPong &s, const Stamps &stamp, int f, int stride,
                           const int *prev_rows, int n_rows, void *stream) {
    const bool in_prompt = f < p->n_prompt;
    const int bound = in_prompt ? p->n_live_host[f] : n_rows;
    if (bound < 0 || (in_prompt && bound > stride)) return -1;
    JLM_TRY(stamp(f, 0));
    if (bound > 0)
        JLM_TRY(rows_lstm_step(m, s.h_in, s.c_in, s.h_out, s.c_out, p->rows, in_prompt ? p->prev + (size_t)f * stride : prev_rows,
                               in_prompt ? p->prompt + (size_t)f * stride : p->word, p->T, bound, in_prompt ? p->n_live + f : nullptr,
                               stream));
    return stamp(f, 1);
}

// The priming loop (include/jlm_hip.h jlm_prime_frames): the LSTM step of the live prefix of right-aligned word rows, frame by frame,
// and nothing else -- the state a decode with a left context starts from.  after_step(f, bound, h_out): called behind the step of
// frame f with the state set it wrote (jlm_prime_cache_frames' copies; jlm_prime_frames: nothing).
template <class AfterStep>
static int prime_loop(const jlm_decode_model *m, const jlm_prime_plan *p, void *stream, AfterStep after_step) {
    const int R = p->n_rows, S = p->n_steps;
    if (R < 0 || S < 0) return -1;
    if (R == 0 || S == 0) return 0;
    if (!p->rows || !p->prev || !p->word || !p->n_live || !p->n_live_host || !p->h[0] || !p->h[1] || !p->c[0] || !p->c[1]) return -1;
    if (m->split_lstm && !m->wt8) return -2;
    for (int f = 0; f < S; ++f) {
        const int bound = p->n_live_host[f];
        if (bound < 0 || bound > R) return -1;
        if (bound == 0) continue;
        JLM_TRY(rows_lstm_step(m, p->h[f & 1], p->c[f & 1], p->h[(f + 1) & 1], p->c[(f + 1) & 1], p->rows, p->prev + (size_t)f * R,
                               p->word + (size_t)f * R, nullptr, bound, p->n_live + f, stream));
        JLM_TRY(after_step(f, bound, p->h[(f + 1) & 1]));
    }
    return 0;
}

extern "C" int jlm_prime_frames(const jlm_decode_model *m, const jlm_prime_plan *p, void *stream) {
    return prime_loop(m, p, stream, [](int, int, const void *) { return 0; });
}

// the copy behind a step: rows 0 .. bound - 1 of the written state set and the step's targets into their ring slot (csrc/jlm_cache.hip)
int jlm_cache_store(const void *h_rows, const int *target, int bound, int H, void *hist_slot, int *words_slot, void *stream);

// Priming that keeps its states (include/jlm_hip.h jlm_prime_cache_frames): prime_loop with the state rows and the targets of the last
// `cap` frames copied into hist / words -- the window of a decode under the continuous cache.
extern "C" int jlm_prime_cache_frames(const jlm_decode_model *m, const jlm_prime_plan *p, const int *target, void *hist, int *words, int cap,
                                      void *stream) {
    if (!p || cap < 1) return -1;
    const int R = p->n_rows, S = p->n_steps;
    if (R > 0 && S > 0 && (!target || !hist || !words || ((uintptr_t)hist & 15) != 0)) return -1;
    return prime_loop(m, p, stream, [&](int f, int bound, const void *h_out) -> int {
        const int slot = f - (S - cap);
        if (slot < 0) return 0;
        return jlm_cache_store(h_out, target + (size_t)f * R, bound, m->H, (char *)hist + (size_t)slot * R * m->H * 4,
                               words + (size_t)slot * R, stream);
    });
}

// seed_context_kernel (include/jlm_hip.h jlm_seed_context): workgroup s gathers the primed state of sentence s behind the plan's pool,
// 16 bytes a lane and trip, and lane 0 writes the root row's prev / word.
__global__ void __launch_bounds__(256) seed_context_kernel(const uint4 *__restrict__ src_h, const uint4 *__restrict__ src_c, int rec,
                                                           const int *__restrict__ last, const int *__restrict__ has, int n_src,
                                                           const int *__restrict__ idx, int beam, long long G, uint4 *__restrict__ dst_h,
                                                           uint4 *__restrict__ dst_c, int *__restrict__ ctx_prev, int *__restrict__ ctx_word) {
    const int s = blockIdx.x;
    const int r = idx[s];
    if (r < 0 || r >= n_src) return;
    const bool state = has[r] != 0;
    if (state) {
        const size_t from = (size_t)r * rec, to = ((size_t)G + s) * rec;
        for (int i = threadIdx.x; i < rec; i += blockDim.x) {
            dst_h[to + i] = src_h[from + i];
            dst_c[to + i] = src_c[from + i];
        }
    }
    if (threadIdx.x == 0) {
        ctx_prev[(size_t)s * beam] = state ? (int)(G + s) : -1;
        ctx_word[(size_t)s * beam] = last[r];
    }
}

extern "C" int jlm_seed_context(const void *src_h, const float *src_c, int H, const int *last, const int *has, int n_src, const int *idx,
                                int n_sent, int beam, long long G, void *dst_h, float *dst_c, int *ctx_prev, int *ctx_word, void *stream) {
    if (n_sent < 0 || n_src < 0 || beam < 1 || H < 4 || H % 4 != 0 || G < 0) return -1;
    if (n_sent == 0) return 0;
    if (!src_h || !src_c || !last || !has || !idx || !dst_h || !dst_c || !ctx_prev || !ctx_word) return -1;
    if ((G + n_sent) * (long long)(H / 4) >= 0x7ffffff0ll) return -1;
    if ((((uintptr_t)src_h | (uintptr_t)src_c | (uintptr_t)dst_h | (uintptr_t)dst_c) & 15) != 0) return -1;
    const int rec = H / 4;
    seed_context_kernel<<<dim3(n_sent), dim3(rec >= 256 ? 256 : (rec + 63) / 64 * 64), 0, (hipStream_t)stream>>>(
        (const uint4 *)src_h, (const uint4 *)src_c, rec, last, has, n_src, idx, beam, G, (uint4 *)dst_h, (uint4 *)dst_c, ctx_prev, ctx_word);
    return (int)hipGetLastError();
}

// The steps of a teacher-forced loop (score_loop, rank_loop) over a plan's live rows, a prefix of its row sets.  Step t: its bound (-1
// for one outside 0 .. n_rows, before anything is recorded), stamp 0, the LSTM step, stamp 1, the T projection, stamp 2; then
// tail(t, bound, ndev, target, s) with the step's live count on the device, its targets and its state sets.
template <class Plan, class Tail>
static int forced_steps(const jlm_decode_model *m, const Plan *p, const Stamps &stamp, void *stream, Tail tail) {
    const int R = p->n_rows;
    for (int t = 0; t < p->n_steps; ++t) {
        const int bound = p->n_live_host ? p->n_live_host[t] : R;
        if (bound < 0 || bound > R) return -1;
        const int *ndev = p->n_live + t;
        const PingPong s(m, p->h, p->c, p->T, t);         // (word[] and prev[] are indexed by the row: g = rows[r] = r)
        JLM_TRY(stamp(t, 0));
        if (bound > 0)
            JLM_TRY(rows_lstm_step(m, s.h_in, s.c_in, s.h_out, s.c_out, p->rows, t == 0 ? p->prev0 : p->rows, p->word + (size_t)t * R, p->T,
                                   bound, ndev, stream));
        JLM_TRY(stamp(t, 1));
        if (bound > 0) JLM_TRY(rows_t_projection(m, s.h_out, p->rows, s.T, bound, ndev, stream));
        JLM_TRY(stamp(t, 2));
        JLM_TRY(tail(t, bound, ndev, p->target + (size_t)t * R, s));
    }
    return 0;
}

// Teacher-forced scoring (include/jlm_hip.h jlm_score_frames): per step the LSTM step of the live rows (a prefix of the row sets),
// T, the full-vocabulary normaliser as the frame loop launches it for kind 0, and the fold into -log p of the target word.
// after_step(t, bound, h_out): called behind step t's last stamp with the state set the step wrote (jlm_score_cache_frames' copies;
// jlm_score_frames: nothing).
template <class AfterStep>
static int score_loop(const jlm_decode_model *m, const jlm_score_plan *p, void *stream, void *const *events, AfterStep after_step) {
    const int R = p->n_rows, S = p->n_steps;
    if (R < 0 || S < 0 || !p->rows || !p->prev0 || !p->word || !p->target || !p->n_live || !p->nll_seq) return -1;
    if (R == 0 || S == 0) return 0;
    JLM_TRY(rows_refuse(m, p->T));
    if (!m->self_norm && (!p->part || p->max_parts < 1)) return -1;
    const Stamps stamp{events, JLM_SCORE_EVENTS_PER_STEP, stream};
    return forced_steps(m, p, stamp, stream, [&](int t, int bound, const int *ndev, const int *target, const PingPong &s) -> int {
        int n_parts = 0;
        if (bound > 0 && !m->self_norm) {
            FullLse fl;
            JLM_TRY(full_lse_pack(m, s.T, p->rows, bound, ndev, p->Tm, p->ld_tm, false, fl, stream));
            JLM_TRY(full_lse_run(m, fl, s.T, s.h_out, p->Tm, p->ld_tm, p->rows, R, bound, bound, ndev, p->part, p->max_parts, 0, &n_parts,
                                 stream));
        }
        JLM_TRY(stamp(t, 3));
        if (bound > 0)
            JLM_TRY(jlm_score_fold(m->segs, m->n_segs, m->b2, s.T, m->ldt, p->part, R, n_parts, m->self_norm, target, ndev, bound,
                                   p->nll_seq, p->nll_tok ? p->nll_tok + (size_t)t * R : nullptr, p->flags, stream));
        JLM_TRY(stamp(t, 4));
        return after_step(t, bound, s.h_out);
    });
}

extern "C" int jlm_score_frames(const jlm_decode_model *m, const jlm_score_plan *p, void *stream, void *const *events) {
    return score_loop(m, p, stream, events, [](int, int, const void *) { return 0; });
}

// Candidate lists behind a static decode (include/jlm_hip.h jlm_alt_frames): alt_head_kernel (csrc/jlm_alt.hip) seeds the accumulator,
// the row sets and prev0 of the plan's rows from the decode's pools, then jlm_score_frames' launches add the suffix terms.  What
// score_loop would refuse at its first step or later is refused here, before the head launch.
extern "C" int jlm_alt_frames(const jlm_decode_model *m, const jlm_alt_plan *a, const jlm_score_plan *p, void *stream, void *const *events) {
    if (!m || !a || !p) return -1;
    const int R = p->n_rows, S = p->n_steps;
    JLM_TRY(jlm_alt_head_refuse(m->segs, m->n_segs, m->b2, m->ldt, m->H, m->self_norm ? 1 : 0, a, p));
    if (R > 0 && S > 0) {
        if (!p->rows || !p->prev0 || !p->word || !p->target || !p->n_live || !p->nll_seq) return -1;
        JLM_TRY(rows_refuse(m, p->T));
        if (!m->self_norm && (!p->part || p->max_parts < 1)) return -1;
        for (int t = 0; t < S; ++t)
            if (p->n_live_host && (p->n_live_host[t] < 0 || p->n_live_host[t] > R)) return -1;
    }
    JLM_TRY(jlm_alt_head(m->segs, m->n_segs, m->b2, m->ldt, m->H, m->self_norm ? 1 : 0, a, p, stream));
    if (R <= 0 || S <= 0) return 0;
    return jlm_score_frames(m, p, stream, events);
}

// the refusals of jlm_cache_rows on their own (csrc/jlm_cache.hip)
int jlm_cache_refuse(const void *hist, const int *words, int cap, int n_rows, int H, int split, float h_scale, int pos0, int n_query,
                     const int *first, const int *len, int N, const float *thetas, int n_theta, const float *lpc);
// the copy behind a step: rows 0 .. bound - 1 of the written state set and the step's targets into their ring slot (csrc/jlm_cache.hip)
int jlm_cache_store(const void *h_rows, const int *target, int bound, int H, void *hist_slot, int *words_slot, void *stream);
// ... of step t of a cached loop over R rows, into slot (pos0 + t) % cap of the plan's rings
template <class CachePlan>
static int ring_store(const CachePlan *cp, int t, const void *h_out, const int *target, int bound, int R, int H, void *stream) {
    const size_t slot = (size_t)((cp->pos0 + t) % cp->cap);
    return jlm_cache_store(h_out, target + (size_t)t * R, bound, H, (char *)cp->hist + slot * R * H * 4, cp->words + slot * R, stream);
}

// Cached scoring (include/jlm_hip.h jlm_score_cache_frames): score_loop with the written state rows and the targets of every step
// copied into the rings, and cache_rows_kernel once behind the last step.
extern "C" int jlm_score_cache_frames(const jlm_decode_model *m, const jlm_score_plan *p, const jlm_cache_plan *cp, void *stream,
                                      void *const *events) {
    if (!cp) return -1;
    const int R = p->n_rows, S = p->n_steps;
    const int split = m->split_lstm ? 1 : 0;
    JLM_TRY(jlm_cache_refuse(cp->hist, cp->words, cp->cap, R, m->H, split, m->h_scale, cp->pos0, S, cp->first, cp->len, cp->N, cp->thetas,
                             cp->n_theta, cp->lpc));
    JLM_TRY(score_loop(m, p, stream, events,
                       [&](int t, int bound, const void *h_out) { return ring_store(cp, t, h_out, p->target, bound, R, m->H, stream); }));
    if (R <= 0 || S <= 0) return 0;
    return jlm_cache_rows(cp->hist, cp->words, cp->cap, R, m->H, split, m->h_scale, cp->pos0, S, cp->first, cp->len, cp->N, cp->thetas,
                          cp->n_theta, cp->lpc, cp->flags, stream);
}

// the refusals of jlm_memory_rows on their own (csrc/jlm_memory.hip)
int jlm_memory_refuse(const void *keys, const int *key_words, int N, int H, int split, float h_scale, const void *q_rows, const int *q_words,
                      int n_rows, int n_steps, const int *len, const float *thetas, int n_theta, const float *lpm, const void *workspace,
                      size_t workspace_bytes, const int *flags);

// Scoring against a memory (include/jlm_hip.h jlm_score_memory_frames): score_loop with jlm_score_cache_frames' store hook over a ring
// of exactly n_steps slots with nothing carried -- the query rows -- and memory_rows_kernel once behind the last step.
extern "C" int jlm_score_memory_frames(const jlm_decode_model *m, const jlm_score_plan *p, const jlm_memory_plan *mp, void *stream,
                                       void *const *events) {
    if (!m || !p || !mp) return -1;
    const int R = p->n_rows, S = p->n_steps;
    const int split = m->split_lstm ? 1 : 0;
    JLM_TRY(jlm_memory_refuse(mp->keys, mp->key_words, mp->N, m->H, split, m->h_scale, mp->q_rows, mp->q_words, R, S, mp->len, mp->thetas,
                              mp->n_theta, mp->lpm, mp->workspace, mp->workspace_bytes, mp->flags));
    struct {
        void *hist; int *words; int cap, pos0;
    } ring{mp->q_rows, mp->q_words, S > 0 ? S : 1, 0};
    JLM_TRY(score_loop(m, p, stream, events,
                       [&](int t, int bound, const void *h_out) { return ring_store(&ring, t, h_out, p->target, bound, R, m->H, stream); }));
    if (R <= 0 || S <= 0) return 0;
    return jlm_memory_rows(mp->keys, mp->key_words, mp->N, m->H, split, m->h_scale, mp->q_rows, mp->q_words, R, S, mp->len, mp->thetas,
                           mp->n_theta, mp->lpm, mp->workspace, mp->workspace_bytes, mp->flags, stream);
}

// Teacher-forced ranking (include/jlm_hip.h jlm_rank_frames): jlm_score_frames' loop over the live rows with the materialised logits
// of a drawing frame of jlm_generate_frames in the normaliser's place, and rank_rows_kernel (csrc/jlm_rank.hip) on the step's targets.
// before_rank(t, bound, h_out, ndev, stamp): between the logit GEMMs' stamp and the ranking, with the state set the step wrote;
// after_rank(t, bound, h_out): behind the ranking, ahead of the step's last stamp, per_step - 1.  jlm_rank_frames: nothing in either;
// jlm_rank_cache_frames: the cache's query and patch (stamps 4 and 5), and the top-k list and the ring write.
template <class BeforeRank, class AfterRank>
static int rank_loop(const jlm_decode_model *m, const jlm_rank_plan *p, void *stream, void *const *events, int per_step,
                     BeforeRank before_rank, AfterRank after_rank) {
    const int R = p->n_rows, S = p->n_steps;
    if (R < 0 || S < 0 || !p->rows || !p->prev0 || !p->word || !p->target || !p->n_live || !p->logits || !p->rank) return -1;
    if (p->n_levels < 0 || p->n_levels > JLM_RANK_MAX_LEVELS) return -1;
    if (R == 0 || S == 0) return 0;
    JLM_TRY(rows_refuse(m, p->T));
    const int V = m->segs[m->n_segs - 1].v_end;
    JLM_TRY(logits_refuse(p->ld_logits, V));
    const Stamps stamp{events, per_step, stream};
    const size_t ld_rank = (size_t)p->n_levels + 1;
    return forced_steps(m, p, stamp, stream, [&](int t, int bound, const int *ndev, const int *target, const PingPong &s) -> int {
        if (bound > 0) JLM_TRY(rows_logits(m, s.T, p->logits, p->ld_logits, bound, stream));
        JLM_TRY(stamp(t, 3));
        JLM_TRY(before_rank(t, bound, s.h_out, ndev, stamp));
        if (bound > 0)
            JLM_TRY(jlm_rank_rows(p->logits, p->ld_logits, V, bound, ndev, target, p->ids, p->n_ids, p->lv_off, p->lv_lo, p->lv_hi, p->n_levels,
                                  p->rank + (size_t)t * R * ld_rank, p->flags, stream));
        JLM_TRY(after_rank(t, bound, s.h_out));
        return stamp(t, per_step - 1);
    });
}

extern "C" int jlm_rank_frames(const jlm_decode_model *m, const jlm_rank_plan *p, void *stream, void *const *events) {
    return rank_loop(m, p, stream, events, JLM_RANK_EVENTS_PER_STEP, [](int, int, const void *, const int *, const Stamps &) { return 0; },
                     [](int, int, const void *) { return 0; });
}

// the refusals of jlm_cache_query / jlm_cache_mix_rows on their own (csrc/jlm_cache_mix.hip)
int jlm_cache_query_refuse(const void *hist, int cap, int n_rows, int H, int split, float h_scale, const void *q_rows, int n_rows_max,
                           const int *n_dev, int pos, const int *first, int N, float theta, const float *s, int ld_s, const int *flags);
int jlm_cache_mix_refuse(const float *y, int ld_y, int n_cols, const float *s, int ld_s, const int *words, int cap, int n_rows,
                         int n_rows_max, const int *n_dev, int pos, const int *first, int N, float lam, const float *lpc_ent,
                         const int *flags);

// Ranking under the continuous cache (include/jlm_hip.h jlm_rank_cache_frames): rank_loop with the logits of every step patched into
// the mixed distribution before they are ranked -- cache_query_kernel on the state set the step wrote, cache_mix_rows_kernel -- an
// optional top-k list of the patched rows, and jlm_score_cache_frames' ring write behind the step.
extern "C" int jlm_rank_cache_frames(const jlm_decode_model *m, const jlm_rank_plan *p, const jlm_cache_mix_plan *cp, void *stream,
                                     void *const *events) {
    if (!cp || !p || m->n_segs < 1) return -1;
    const int R = p->n_rows, S = p->n_steps;
    if (R < 0 || S < 0 || cp->pos0 < 0 || (long long)cp->pos0 + S > 0x7fffffffll) return -1;
    const int split = m->split_lstm ? 1 : 0;
    const int V = m->segs[m->n_segs - 1].v_end;
    const int pos_last = cp->pos0 + (S > 0 ? S - 1 : 0);
    JLM_TRY(jlm_cache_query_refuse(cp->hist, cp->cap, R, m->H, split, m->h_scale, p->h[0], R, p->n_live, pos_last, cp->first, cp->N, cp->theta,
                                   cp->s, cp->ld_s, cp->flags));
    JLM_TRY(jlm_cache_mix_refuse(p->logits, p->ld_logits, V, cp->s, cp->ld_s, cp->words, cp->cap, R, R, p->n_live, pos_last, cp->first, cp->N,
                                 cp->lam, nullptr, cp->flags));
    if (cp->top_k < 0 || cp->top_k > JLM_TOPK_MAX || cp->top_k > V) return -1;
    if (cp->top_k > 0 && (!cp->top_ids || !cp->top_nll || !p->n_live_host)) return -1;
    if (p->n_live_host)
        for (int t = 0; t < S; ++t)
            if (p->n_live_host[t] < 0 || p->n_live_host[t] > R) return -1;
    return rank_loop(
        m, p, stream, events, JLM_RANK_CACHE_EVENTS_PER_STEP,
        [&](int t, int bound, const void *h_out, const int *ndev, const Stamps &stamp) -> int {
            const int pos = cp->pos0 + t;
            if (bound > 0)
                JLM_TRY(jlm_cache_query(cp->hist, cp->cap, R, m->H, split, m->h_scale, h_out, bound, ndev, pos, cp->first, cp->N, cp->theta,
                                        cp->s, cp->ld_s, cp->flags, stream));
            JLM_TRY(stamp(t, 4));
            if (bound > 0)
                JLM_TRY(jlm_cache_mix_rows(p->logits, p->ld_logits, V, m->self_norm, cp->s, cp->ld_s, cp->words, cp->cap, R, bound, ndev, pos,
                                           cp->first, cp->N, cp->lam, nullptr, cp->flags, stream));
            return stamp(t, 5);
        },
        [&](int t, int bound, const void *h_out) -> int {
            if (cp->top_k > 0 && p->n_live_host[t] > 0)
                JLM_TRY(jlm_topk_rows(p->logits, p->ld_logits, V, p->n_live_host[t], cp->top_k, m->self_norm,
                                      cp->top_ids + (size_t)t * R * cp->top_k, cp->top_nll + (size_t)t * R * cp->top_k, cp->top_k, p->flags,
                                      stream));
            return ring_store(cp, t, h_out, p->target, bound, R, m->H, stream);
        });
}

// Ranking under the n-gram mixture (include/jlm_hip.h jlm_rank_ngram_frames): rank_loop with ngram_mix_rows_kernel on every step's
// logits before they are ranked, and an optional top-k list of the patched rows behind the ranking.  The loop is teacher-forced, so
// the host knows every history and uploads them: nothing is carried on the device.
extern "C" int jlm_rank_ngram_frames(const jlm_decode_model *m, const jlm_rank_plan *p, const jlm_ngram_mix_plan *np, void *stream,
                                     void *const *events) {
    if (!np || !p || !m || m->n_segs < 1) return -1;
    const int R = p->n_rows, S = p->n_steps;
    if (R < 0 || S < 0) return -1;
    const int V = m->segs[m->n_segs - 1].v_end;
    JLM_TRY(jlm_ngram_mix_refuse(p->logits, p->ld_logits, V, np->table, np->hist, R, p->n_live, np->lam, np->order, np->flags));
    if (np->top_k < 0 || np->top_k > JLM_TOPK_MAX || np->top_k > V) return -1;
    if (np->top_k > 0 && (!np->top_ids || !np->top_nll || !p->n_live_host)) return -1;
    // (with the logits checked by the patch's refusals above, that is every -1 of jlm_topk_rows: nothing is left to refuse in the loop)
    if (p->n_live_host)
        for (int t = 0; t < S; ++t)
            if (p->n_live_host[t] < 0 || p->n_live_host[t] > R) return -1;
    return rank_loop(
        m, p, stream, events, JLM_RANK_NGRAM_EVENTS_PER_STEP,
        [&](int t, int bound, const void *, const int *ndev, const Stamps &stamp) -> int {
            if (bound > 0)
                JLM_TRY(jlm_ngram_mix_rows(p->logits, p->ld_logits, V, m->self_norm, np->table, np->hist + (size_t)t * R * 2, bound, ndev,
                                           np->lam, np->order, np->flags, stream));
            return stamp(t, 4);
        },
        [&](int t, int, const void *) -> int {
            if (np->top_k > 0 && p->n_live_host[t] > 0)
                JLM_TRY(jlm_topk_rows(p->logits, p->ld_logits, V, p->n_live_host[t], np->top_k, m->self_norm,
                                      np->top_ids + (size_t)t * R * np->top_k, np->top_nll + (size_t)t * R * np->top_k, np->top_k, p->flags,
                                      stream));
            return 0;
        });
}

// One step of prediction under the cache, for a caller who holds the carried state of its streams (include/jlm_hip.h
// jlm_predict_cache_rows): the T projection of h, the logits, the cache's query and patch at `pos`, and the (masked) top-k selection.
// No LSTM step and no ring write.
extern "C" int jlm_predict_cache_rows(const jlm_decode_model *m, const jlm_predict_cache_plan *p, void *stream) {
    if (!p || m->n_segs < 1) return -1;
    const int R = p->n_rows;
    if (R < 0 || !p->rows || !p->logits || !p->ids || !p->nll) return -1;
    if (m->untied && m->split_lstm) return -2;                     // its vocabulary GEMMs read the f32 copy only the LSTM step writes
    const int split = m->split_lstm ? 1 : 0;
    const int V = m->segs[m->n_segs - 1].v_end;
    JLM_TRY(jlm_cache_query_refuse(p->hist, p->cap, R, m->H, split, m->h_scale, p->h, R, nullptr, p->pos, p->first, p->N, p->theta, p->s,
                                   p->ld_s, p->cache_flags));
    JLM_TRY(jlm_cache_mix_refuse(p->logits, p->ld_logits, V, p->s, p->ld_s, p->words, p->cap, R, R, nullptr, p->pos, p->first, p->N, p->lam,
                                 nullptr, p->cache_flags));
    if (p->k < 1 || p->k > JLM_TOPK_MAX || p->k > V) return -1;
    if (p->row_set && (p->n_sets < 0 || (p->n_sets > 0 && (!p->mask || p->ld_mask < (V + 31) / 32)))) return -1;
    if (R == 0) return 0;
    JLM_TRY(rows_refuse(m, p->T));
    float *T = t_is_state(m) ? (float *)const_cast<void *>(p->h) : p->T;
    JLM_TRY(rows_t_projection(m, const_cast<void *>(p->h), p->rows, T, R, nullptr, stream));
    JLM_TRY(rows_logits(m, T, p->logits, p->ld_logits, R, stream));
    JLM_TRY(jlm_cache_query(p->hist, p->cap, R, m->H, split, m->h_scale, p->h, R, nullptr, p->pos, p->first, p->N, p->theta, p->s, p->ld_s,
                            p->cache_flags, stream));
    JLM_TRY(jlm_cache_mix_rows(p->logits, p->ld_logits, V, m->self_norm, p->s, p->ld_s, p->words, p->cap, R, R, nullptr, p->pos, p->first,
                               p->N, p->lam, nullptr, p->cache_flags, stream));
    if (p->row_set)
        return jlm_topk_rows_masked(p->logits, p->ld_logits, V, R, p->k, m->self_norm, p->mask, p->ld_mask, p->n_sets, p->row_set, p->ids,
                                    p->nll, p->k, p->flags, stream);
    return jlm_topk_rows(p->logits, p->ld_logits, V, R, p->k, m->self_norm, p->ids, p->nll, p->k, p->flags, stream);
}

// Ranking under a memory (include/jlm_hip.h jlm_rank_memory_frames): rank_loop with the logits of every step patched into the mixed
// distribution before they are ranked -- the retrieval on the state set the step wrote, then cache_mix_rows_kernel over the retrieved
// entries as a window of min(K, N) positions in a ring of K slots -- and an optional top-k list of the patched rows.
extern "C" int jlm_rank_memory_frames(const jlm_decode_model *m, const jlm_rank_plan *p, const jlm_memory_mix_plan *mp, void *stream,
                                      void *const *events) {
    if (!m || !p || !mp || m->n_segs < 1) return -1;
    const int R = p->n_rows, S = p->n_steps;
    if (R < 0 || S < 0) return -1;
    const int split = m->split_lstm ? 1 : 0;
    const int V = m->segs[m->n_segs - 1].v_end;
    JLM_TRY(jlm_memory_topk_refuse(mp->keys, mp->key_words, mp->N, m->H, split, m->h_scale, p->h[0], R, p->n_live, mp->theta, mp->K, mp->s,
                                   mp->ld_s, mp->ret_words, mp->ret_idx, R, mp->workspace, mp->workspace_bytes, mp->flags));
    const int n_q = mp->K < mp->N ? mp->K : mp->N;
    JLM_TRY(jlm_cache_mix_refuse(p->logits, p->ld_logits, V, mp->s, mp->ld_s, mp->ret_words, mp->K, R, R, p->n_live, n_q, mp->first, mp->K,
                                 mp->lam, nullptr, mp->flags));
    if (mp->keep_idx && !mp->ret_idx) return -1;
    if (mp->top_k < 0 || mp->top_k > JLM_TOPK_MAX || mp->top_k > V) return -1;
    if (mp->top_k > 0 && (!mp->top_ids || !mp->top_nll || !p->n_live_host)) return -1;
    if (p->n_live_host)
        for (int t = 0; t < S; ++t)
            if (p->n_live_host[t] < 0 || p->n_live_host[t] > R) return -1;
    return rank_loop(
        m, p, stream, events, JLM_RANK_MEMORY_EVENTS_PER_STEP,
        [&](int t, int bound, const void *h_out, const int *ndev, const Stamps &stamp) -> int {
            int *idx = mp->keep_idx ? mp->ret_idx + (size_t)t * mp->K * R : mp->ret_idx;
            if (bound > 0)
                JLM_TRY(jlm_memory_topk(mp->keys, mp->key_words, mp->N, m->H, split, m->h_scale, h_out, bound, ndev, mp->theta, mp->K, mp->s,
                                        mp->ld_s, mp->ret_words, idx, R, mp->workspace, mp->workspace_bytes, mp->flags, stream));
            JLM_TRY(stamp(t, 4));
            if (bound > 0)
                JLM_TRY(jlm_cache_mix_rows(p->logits, p->ld_logits, V, m->self_norm, mp->s, mp->ld_s, mp->ret_words, mp->K, R, bound, ndev, n_q,
                                           mp->first, mp->K, mp->lam, nullptr, mp->flags, stream));
            return stamp(t, 5);
        },
        [&](int t, int, const void *) -> int {
            if (mp->top_k > 0 && p->n_live_host[t] > 0)
                JLM_TRY(jlm_topk_rows(p->logits, p->ld_logits, V, p->n_live_host[t], mp->top_k, m->self_norm,
                                      mp->top_ids + (size_t)t * R * mp->top_k, mp->top_nll + (size_t)t * R * mp->top_k, mp->top_k, p->flags,
                                      stream));
            return 0;
        });
}

// One step of prediction under a memory (include/jlm_hip.h jlm_predict_memory_rows): jlm_predict_cache_rows with the retrieval in the
// query's place.  No LSTM step.
extern "C" int jlm_predict_memory_rows(const jlm_decode_model *m, const jlm_predict_memory_plan *p, void *stream) {
    if (!m || !p || m->n_segs < 1) return -1;
    const int R = p->n_rows;
    if (R < 0 || !p->rows || !p->logits || !p->ids || !p->nll) return -1;
    if (m->untied && m->split_lstm) return -2;                     // its vocabulary GEMMs read the f32 copy only the LSTM step writes
    const int split = m->split_lstm ? 1 : 0;
    const int V = m->segs[m->n_segs - 1].v_end;
    JLM_TRY(jlm_memory_topk_refuse(p->keys, p->key_words, p->N, m->H, split, m->h_scale, p->h, R, nullptr, p->theta, p->K, p->s, p->ld_s,
                                   p->ret_words, p->ret_idx, R, p->workspace, p->workspace_bytes, p->memory_flags));
    const int n_q = p->K < p->N ? p->K : p->N;
    JLM_TRY(jlm_cache_mix_refuse(p->logits, p->ld_logits, V, p->s, p->ld_s, p->ret_words, p->K, R, R, nullptr, n_q, p->first, p->K, p->lam,
                                 nullptr, p->memory_flags));
    if (p->k < 1 || p->k > JLM_TOPK_MAX || p->k > V) return -1;
    if (p->row_set && (p->n_sets < 0 || (p->n_sets > 0 && (!p->mask || p->ld_mask < (V + 31) / 32)))) return -1;
    if (R == 0) return 0;
    JLM_TRY(rows_refuse(m, p->T));
    float *T = t_is_state(m) ? (float *)const_cast<void *>(p->h) : p->T;
    JLM_TRY(rows_t_projection(m, const_cast<void *>(p->h), p->rows, T, R, nullptr, stream));
    JLM_TRY(rows_logits(m, T, p->logits, p->ld_logits, R, stream));
    JLM_TRY(jlm_memory_topk(p->keys, p->key_words, p->N, m->H, split, m->h_scale, p->h, R, nullptr, p->theta, p->K, p->s, p->ld_s, p->ret_words,
                            p->ret_idx, R, p->workspace, p->workspace_bytes, p->memory_flags, stream));
    JLM_TRY(jlm_cache_mix_rows(p->logits, p->ld_logits, V, m->self_norm, p->s, p->ld_s, p->ret_words, p->K, R, R, nullptr, n_q, p->first, p->K,
                               p->lam, nullptr, p->memory_flags, stream));
    if (p->row_set)
        return jlm_topk_rows_masked(p->logits, p->ld_logits, V, R, p->k, m->self_norm, p->mask, p->ld_mask, p->n_sets, p->row_set, p->ids,
                                    p->nll, p->k, p->flags, stream);
    return jlm_topk_rows(p->logits, p->ld_logits, V, R, p->k, m->self_norm, p->ids, p->nll, p->k, p->flags, stream);
}

// Ancestral sampling (include/jlm_hip.h jlm_generate_frames): the prompt frames step the LSTM of their live prefix only; every drawing
// frame steps all rows, projects T, materialises the full-vocabulary logits (one jlm_gemm_nt per segment, columns v_start .. v_end of
// plan.logits, + b2) and draws with sample_rows_kernel, which also writes the word the next frame consumes.  With top_k / top_p on
// (jlm_generate_frames_trunc) the draw is sample_rows_trunc_kernel's; jlm_sample_rows_trunc launches the untruncated kernel when
// both are off.
static int generate_frames(const jlm_decode_model *m, const jlm_generate_plan *p, int top_k, double top_p, void *stream,
                           void *const *events) {
    const int R = p->n_rows, P = p->n_prompt, N = p->n_words;
    if (R < 0 || P < 1 || N < 0 || !p->rows || !p->prev || !p->prompt || !p->n_live || !p->n_live_host || !p->word || !p->ids || !p->nll ||
        !p->logits)
        return -1;
    if (R == 0 || N == 0) return 0;
    JLM_TRY(rows_refuse(m, p->T));
    const int V = m->segs[m->n_segs - 1].v_end;
    JLM_TRY(logits_refuse(p->ld_logits, V));
    if (p->n_live_host[P - 1] != R) return -1;                  // every row is live at the last prompt frame (right-aligned prompts)
    const Stamps stamp{events, JLM_GENERATE_EVENTS_PER_FRAME, stream};
    const int F = P + N - 1;
    for (int f = 0; f < F; ++f) {
        const PingPong s(m, p->h, p->c, p->T, f);
        JLM_TRY(frame_lstm_step(m, p, s, stamp, f, R, p->rows, R, stream));
        const int k = f - (P - 1);                                   // the draw of this frame, if any
        if (k >= 0) JLM_TRY(rows_t_projection(m, s.h_out, p->rows, s.T, R, nullptr, stream));
        JLM_TRY(stamp(f, 2));
        if (k >= 0) JLM_TRY(rows_logits(m, s.T, p->logits, p->ld_logits, R, stream));
        JLM_TRY(stamp(f, 3));
        if (k >= 0)
            JLM_TRY(jlm_sample_rows_trunc(p->logits, p->ld_logits, V, R, nullptr, p->temperature, p->seed, k, p->row_id, nullptr, p->done,
                                          p->stop_id, m->self_norm, top_k, top_p, p->word, p->ids + (size_t)k * R,
                                          p->nll + (size_t)k * R, p->flags, stream));
        JLM_TRY(stamp(f, 4));
    }
    return 0;
}

extern "C" int jlm_generate_frames(const jlm_decode_model *m, const jlm_generate_plan *p, void *stream, void *const *events) {
    return generate_frames(m, p, 0, 1.0, stream, events);
}

extern "C" int jlm_generate_frames_trunc(const jlm_decode_model *m, const jlm_generate_plan *p, int top_k, double top_p, void *stream,
                                         void *const *events) {
    if (!(top_p > 0.0)) return -1;
    return generate_frames(m, p, top_k, top_p, stream, events);
}

// Beam-search completion (include/jlm_hip.h jlm_complete_frames): the prompt frames as jlm_generate_frames' over the n_prompts prompt
// rows; selecting frame 0 projects, materialises and selects from those rows alone (a prompt's beam starts from its one
// distribution); every later frame steps all n_prompts * beam rows from the rows the previous merge chose, then the T projection, the
// logit GEMMs, topk_rows_kernel and beam_merge_kernel, which writes the next frame's word / prev row and the back-pointers.
// prompt_set (jlm_complete_frames_masked; NULL: none): selecting frame 0's rows, one per prompt, select within their word sets.
// before_select(k, n_sel): between the logit GEMMs' stamp and selecting frame k's selection; after_merge(k, n_sel): behind its merge,
// ahead of the frame's last stamp.  jlm_complete_frames and jlm_complete_frames_masked: nothing in either -- the same launches in the
// same order --; jlm_complete_frames_ngram: the n-gram patch of the n_sel rows, and the histories of the rows the merge wrote.
template <class BeforeSelect, class AfterMerge>
static int complete_frames(const jlm_decode_model *m, const jlm_complete_plan *p, const unsigned *mask, int ld_mask, int n_sets,
                           const int *prompt_set, void *stream, void *const *events, BeforeSelect before_select, AfterMerge after_merge) {
    const int NP = p->n_prompts, B = p->beam, P = p->n_prompt, N = p->n_words;
    if (NP < 0 || B < 1 || B > JLM_TOPK_MAX || P < 1 || N < 0 || !p->rows || !p->prev || !p->prompt || !p->n_live || !p->n_live_host ||
        !p->logits || !p->cand_ids || !p->cand_nll || !p->word || !p->prev_row || !p->score || !p->finished || !p->bp_parent ||
        !p->bp_word || !p->bp_nll)
        return -1;
    if (NP == 0 || N == 0) return 0;
    JLM_TRY(rows_refuse(m, p->T));
    const int V = m->segs[m->n_segs - 1].v_end;
    if (B > V || (long long)NP * B > 0x7fffffff) return -1;
    const int R = NP * B;
    JLM_TRY(logits_refuse(p->ld_logits, V));
    if (p->n_live_host[P - 1] != NP) return -1;                 // every prompt is live at the last prompt frame (right-aligned)
    const Stamps stamp{events, JLM_COMPLETE_EVENTS_PER_FRAME, stream};
    const int F = P + N - 1;
    for (int f = 0; f < F; ++f) {
        const PingPong s(m, p->h, p->c, p->T, f);
        JLM_TRY(frame_lstm_step(m, p, s, stamp, f, NP, p->prev_row, R, stream));
        const int k = f - (P - 1);                                   // the selecting frame, if any
        const int n_sel = k == 0 ? NP : R;
        if (k >= 0) JLM_TRY(rows_t_projection(m, s.h_out, p->rows, s.T, n_sel, nullptr, stream));
        JLM_TRY(stamp(f, 2));
        if (k >= 0) JLM_TRY(rows_logits(m, s.T, p->logits, p->ld_logits, n_sel, stream));
        JLM_TRY(stamp(f, 3));
        if (k >= 0) JLM_TRY(before_select(k, n_sel));
        if (k == 0 && prompt_set)
            JLM_TRY(jlm_topk_rows_masked(p->logits, p->ld_logits, V, n_sel, B, m->self_norm, mask, ld_mask, n_sets, prompt_set, p->cand_ids,
                                         p->cand_nll, B, p->flags, stream));
        else if (k >= 0)
            JLM_TRY(jlm_topk_rows(p->logits, p->ld_logits, V, n_sel, B, m->self_norm, p->cand_ids, p->cand_nll, B, p->flags, stream));
        JLM_TRY(stamp(f, 4));
        if (k >= 0)
            JLM_TRY(jlm_beam_merge(p->cand_ids, p->cand_nll, B, NP, k == 0, p->stop_id, p->word, p->prev_row, p->score, p->finished,
                                   p->bp_parent + (size_t)k * R, p->bp_word + (size_t)k * R, p->bp_nll + (size_t)k * R, stream));
        if (k >= 0) JLM_TRY(after_merge(k, n_sel));
        JLM_TRY(stamp(f, 5));
    }
    return 0;
}

extern "C" int jlm_complete_frames(const jlm_decode_model *m, const jlm_complete_plan *p, void *stream, void *const *events) {
    return complete_frames(m, p, nullptr, 0, 0, nullptr, stream, events, [](int, int) { return 0; }, [](int, int) { return 0; });
}

extern "C" int jlm_complete_frames_masked(const jlm_decode_model *m, const jlm_complete_plan *p, const unsigned *mask, int ld_mask,
                                          int n_sets, const int *prompt_set, void *stream, void *const *events) {
    if (!prompt_set || n_sets < 0 || (n_sets > 0 && !mask)) return -1;
    return complete_frames(m, p, mask, ld_mask, n_sets, prompt_set, stream, events, [](int, int) { return 0; }, [](int, int) { return 0; });
}

// Completion under the n-gram mixture (include/jlm_hip.h jlm_complete_frames_ngram): complete_frames with the n_sel rows of every
// selecting frame patched by ngram_mix_rows_kernel before the selection, plain or masked, and ngram_hist_advance_kernel behind every
// merge but the last: hist[(k + 1) & 1] of the rows the merge wrote from hist[k & 1] of the rows it chose them from.
extern "C" int jlm_complete_frames_ngram(const jlm_decode_model *m, const jlm_complete_plan *p, const jlm_complete_ngram_plan *np,
                                         const unsigned *mask, int ld_mask, int n_sets, const int *prompt_set, void *stream,
                                         void *const *events) {
    if (!m || !p || !np || m->n_segs < 1) return -1;
    if (prompt_set ? (n_sets < 0 || (n_sets > 0 && !mask)) : (mask != nullptr || n_sets != 0)) return -1;
    const int NP = p->n_prompts, B = p->beam;
    if (NP < 0 || B < 1 || (long long)NP * B > 0x7fffffff) return -1;
    const int R = NP * B, V = m->segs[m->n_segs - 1].v_end;
    JLM_TRY(jlm_ngram_mix_refuse(p->logits, p->ld_logits, V, np->table, np->hist[0], R, nullptr, np->lam, np->order, np->flags));
    if (R > 0 && p->n_words > 1 && (!np->hist[1] || np->hist[1] == np->hist[0] || (((uintptr_t)np->hist[0] | (uintptr_t)np->hist[1]) & 7) != 0))
        return -1;
    return complete_frames(
        m, p, mask, ld_mask, n_sets, prompt_set, stream, events,
        [&](int k, int n_sel) -> int {
            return jlm_ngram_mix_rows(p->logits, p->ld_logits, V, m->self_norm, np->table, np->hist[k & 1], n_sel, nullptr, np->lam, np->order,
                                      np->flags, stream);
        },
        [&](int k, int n_sel) -> int {
            if (k + 1 >= p->n_words) return 0;
            return jlm_ngram_hist_advance(np->hist[k & 1], n_sel, p->prev_row, p->word, R, np->hist[(k + 1) & 1], stream);
        });
}
