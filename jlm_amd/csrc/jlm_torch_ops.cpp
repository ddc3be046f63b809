// jlm_torch_ops.cpp -- the PyTorch-ROCm custom-op boundary of the decode path.
//
// A thin TORCH_LIBRARY shim over the C-ABI launchers of libjlm_hip.so (include/jlm_hip.h): torch owns every device buffer,
// the ops take torch.Tensor arguments (never raw pointers from Python), launch on the CURRENT torch HIP stream of the
// tensors' device, and turn a non-zero return into a c10::Error (TORCH_CHECK) carrying hipGetErrorString.  What it
// replaces on the reference's side are the call sites decoder/decoder.py:202-218 -> decoder/model.py:195-198
// (Decoder._batch_predict -> LSTM_Model.predict_with_context) and the frame loop around them (decoder.py:220-241).
//
//   torch.classes.jlm.Model   the model's weight panels as jlm_decode_model (keeps the tensors alive)
//   torch.classes.jlm.Plan    the buffers of one decode shape as jlm_lattice / jlm_beam_state / jlm_decode_plan,
//                             plus the timing events of a timed decode
//   torch.ops.jlm.decode_frames(Model, Plan, n_frames, vs_max, di_max, dd_max, use_side, timed, lse_cu_share_pct)
//                             the whole frame loop of a batch: ONE op (jlm_decode_frames)
//   torch.ops.jlm.decode_batch(Model, Plan, staging block, lattice block, read-back buffers, ...)
//                             round 5: upload + frame loop + read-back of one batch, ONE op (what DecodeEngine submits)
//   torch.ops.jlm.frame_times(Plan) -> Tensor [n_frames, 5] milliseconds of the last timed decode (after it finished)
//   torch.ops.jlm.score_frames(Model, state row sets, ..., word, target, n_live, nll outputs, ...)
//                             teacher-forced scoring of many sequences: ONE op (jlm_score_frames; LSTM_Model.score)
//   torch.ops.jlm.sample_rows(y, ..., word, ids, nll, flags)   one draw per row of materialised logits (jlm_sample_rows)
//   torch.ops.jlm.generate_frames(Model, state row sets, logits, prompt arrays, ..., ids, nll, ...)
//                             batched ancestral sampling: ONE op (jlm_generate_frames; LSTM_Model.generate)
//   torch.ops.jlm.sample_rows_trunc / generate_frames_trunc(..., top_k, top_p, ...)
//                             the same two with a top-k / nucleus cut of every draw (jlm_sample_rows_trunc, jlm_generate_frames_trunc)
//   torch.ops.jlm.topk_rows(y, ..., k, ids, nll, flags)        the k best words of every row of materialised logits (jlm_topk_rows)
//   torch.ops.jlm.beam_merge(cand_ids, cand_nll, ...)          one beam selection per prompt (jlm_beam_merge)
//   torch.ops.jlm.complete_frames(Model, state row sets, logits, prompt arrays, ..., back-pointers, ...)
//                             beam-search completion: ONE op (jlm_complete_frames; LSTM_Model.complete / predict_top)
//   torch.ops.jlm.topk_rows_masked / complete_frames_masked(..., mask, ld_mask, n_sets, row_set / prompt_set)
//                             the same two with rows / first words restricted to word sets (jlm_topk_rows_masked,
//                             jlm_complete_frames_masked; LSTM_Model.predict_reading / complete_reading)
//   torch.ops.jlm.rank_rows(y, ..., target, ids, lv_off, lv_lo, lv_hi, n_levels, rank, flags)
//                             the rank of a given word in every row of materialised logits, at every level of its list (jlm_rank_rows)
//   torch.ops.jlm.rank_frames(Model, state row sets, logits, ..., word, target, n_live, level table, rank, ...)
//                             teacher-forced ranking of many sequences: ONE op (jlm_rank_frames; LSTM_Model.rank / rank_streams)
//   torch.ops.jlm.rank_cache_frames / predict_cache_rows
//                             the same under the continuous cache, and its one-step prediction form (jlm_rank_cache_frames,
//                             jlm_predict_cache_rows; LSTM_Model.rank_streams_cached / rank_cached / predict_next_cached)
//   torch.ops.jlm.memory_topk(keys, key_words, ..., q_rows, theta, K, s, ret_words, ret_idx, workspace, flags)
//                             the K nearest entries of a memory for every query row (jlm_memory_topk; Memory.search)
//   torch.ops.jlm.rank_memory_frames / predict_memory_rows
//                             rank_frames under a memory's K nearest entries, and its one-step prediction form (jlm_rank_memory_frames,
//                             jlm_predict_memory_rows; LSTM_Model.rank_streams_memory / rank_memory / predict_next_memory)
//   torch.ops.jlm.prime_frames(Model, state row sets, rows, prev, word, n_live, ...)
//                             the state after a left context: LSTM steps only, ONE op (jlm_prime_frames; LSTM_Model.prime)
//   torch.ops.jlm.seed_context(Plan, src_h, src_c, last, has, idx)
//                             primed states gathered behind a plan's pool for frame 0 (jlm_seed_context; Decoder.decode(context=))
//   torch.ops.jlm.prime_cache_frames(Model, state row sets, ..., target, hist, words, cap)
//                             prime_frames that keeps the last cap frames' states and targets (jlm_prime_cache_frames; prime(cache=))
//   torch.ops.jlm.seed_cache(Plan, hist, words, count, idx, s, cap, N, theta, lam)
//                             the window of the plan's next frame loop: no launch (jlm_decode_plan.cache; Decoder.decode(cache=))
//   torch.ops.jlm.seed_ngram(Plan, keys, vals, root_hist, log2cap, max_probe, order, lam) / clear_ngram(Plan)
//                             the n-gram table of the plan's next frame loop: no launch (jlm_decode_plan.ngram; Decoder.decode(ngram=))
//   torch.ops.jlm.seed_memory(Plan, keys, key_words, N, H, theta, lam, K, q_rows, s, ret_words, workspace, flags) / clear_memory(Plan)
//                             the memory of the plan's next frame loop: no launch (jlm_decode_plan.memory; Decoder.decode(memory=))
//   torch.ops.jlm.alt_frames(Model, Plan, rank, sent_off, sent_rows, depth, alt, score_frames' arguments)
//                             per-segment candidate lists behind a plan's decode (jlm_alt_frames; Decoder.decode_candidates)
//   torch.ops.jlm.tail_predict(Model, Plan, ids, sp_off, sp_frame, sp_lo, sp_hi, n_out, chunk, out_score, out_row, out_word, out_nodes,
//                              out_len, stride)
//                             predictions of an unfinished last word behind a plan's decode (jlm_tail_predict; Decoder.decode_predict)
//   torch.ops.jlm.kmeans1d(x, bit, seed, max_iter, tol, code, codebook, scratch, grid, timed)
//                             scalar k-means compression of one weight tensor: ONE op (jlm_kmeans1d; jlm_amd/compress.py)
//   torch.ops.jlm.train_*       the kernels of a training step, one op per launcher (jlm_train.hip; jlm_amd/train.py DeviceStepper)
//   torch.ops.jlm.train_expand_codes / train_codebook_grad
//                               fine-tuning the codebooks of a compressed model (jlm_amd/finetune.py CodebookDeviceStepper)
//   torch.ops.jlm.train_gemm_splitk / dyneval_sqacc / dyneval_rms / dyneval_update
//                               dynamic evaluation (jlm_amd/dyneval.py DynEvalDeviceStepper)
//   torch.ops.jlm.lstm_step / gemm_nt / softmax_rows     LSTM_Model.predict / project (numpy-facing API)
//   torch.ops.jlm.pack_split_f16 / pack_split_f16_col / dequant_u8     weight preparation at load
//
// Built by __graft_entry__.build():  g++ -shared ... -> jlm_amd/_torch_ops.so, loaded with torch.ops.load_library.
#include <torch/library.h>
#include <torch/custom_class.h>
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>
#include <c10/hip/HIPGuard.h>
#include <hip/hip_runtime_api.h>

#include <array>
#include <map>
#include <mutex>
#include <set>
#include <string>
#include <vector>

#include "../../include/jlm_hip.h"

namespace {

using at::Tensor;
using OptTensor = c10::optional<Tensor>;
using TDict = c10::Dict<std::string, Tensor>;
using IDict = c10::Dict<std::string, int64_t>;
using FDict = c10::Dict<std::string, double>;

void jlm_check(int rc, const char *what) {
    if (rc == 0) return;
    if (rc > 0)
        TORCH_CHECK(false, what, " failed: ", hipGetErrorString(static_cast<hipError_t>(rc)), " (hipError_t ", rc, ")");
    TORCH_CHECK(false, what, " rejected its arguments (code ", rc,
                ": -1 = shape / alignment the kernels cannot handle, -2 = outside the shapes this entry point covers, "
                "-3 = the kernel's LDS size could not be set; include/jlm_hip.h)");
}

void on_gpu(const Tensor &t, const char *name) {
    TORCH_CHECK(t.defined() && t.is_cuda(), "jlm: `", name, "` must be a tensor on the GPU (there is no CPU path)");
    TORCH_CHECK(t.is_contiguous(), "jlm: `", name, "` must be contiguous");
}

template <class T = void> T *ptr(const Tensor &t, const char *name) {
    on_gpu(t, name);
    return reinterpret_cast<T *>(t.data_ptr());
}
template <class T = void> T *optr(const OptTensor &t, const char *name) {
    if (!t.has_value() || !t->defined()) return nullptr;
    return ptr<T>(*t, name);
}

// what the ops' argument checks ask of a tensor: of type `ty` with n elements or more; an optional one: given; given and so, or not given
bool is(const Tensor &t, at::ScalarType ty, int64_t n) { return t.defined() && t.scalar_type() == ty && t.numel() >= n; }
bool has(const OptTensor &t) { return t.has_value() && t->defined(); }
bool opt_ok(const OptTensor &t, at::ScalarType ty, int64_t n) { return !has(t) || is(*t, ty, n); }

// the current torch stream of the device the tensor lives on (ops never switch devices themselves: the caller's
// torch.cuda.device context / set_device is what the HIP runtime launches on)
hipStream_t stream_of(const Tensor &t) { return c10::hip::getCurrentHIPStream(t.device().index()).stream(); }

struct Segments {
    std::vector<jlm_segment> v;
    std::vector<Tensor> keep;
    Segments() = default;
    // meta: (v_start, v_end, k, t_off, ldb) per segment
    Segments(const std::vector<Tensor> &B, const std::vector<int64_t> &meta) : keep(B) {
        TORCH_CHECK(meta.size() == 5 * B.size() && B.size() <= JLM_MAX_SEGMENTS, "jlm: malformed segment table");
        for (size_t i = 0; i < B.size(); ++i) {
            jlm_segment s;
            s.v_start = (int)meta[5 * i]; s.v_end = (int)meta[5 * i + 1]; s.k = (int)meta[5 * i + 2];
            s.t_off = (int)meta[5 * i + 3]; s.ldb = (int)meta[5 * i + 4];
            s.B = ptr<const float>(B[i], "segment block");
            v.push_back(s);
        }
    }
};

const Tensor *find(const TDict &d, const char *key) {
    auto it = d.find(key);
    return it == d.end() ? nullptr : &it->value();
}
int64_t geti(const IDict &d, const char *key, int64_t dflt = 0) {
    auto it = d.find(key);
    return it == d.end() ? dflt : it->value();
}
double getf(const FDict &d, const char *key, double dflt = 0.0) {
    auto it = d.find(key);
    return it == d.end() ? dflt : it->value();
}
template <class T = void> T *tptr(const TDict &d, const char *key) {
    const Tensor *t = find(d, key);
    return t ? ptr<T>(*t, key) : nullptr;
}

// ------------------------------------------------------------------------------------------------- Model
struct JlmModel : torch::CustomClassHolder {
    TDict tensors;
    Segments segs, split, mixed_some;
    std::vector<float> t_scale, descale;
    std::vector<int> bias_col;
    std::vector<jlm_segment> mixed;                 // n_segs entries, B == NULL where the segment has no mixed rows
    std::vector<float> mx_t_scale, mx_descale, mx_s8;
    std::vector<int> mx_head_split;                 // n_segs entries (ABI 10)
    jlm_decode_model m{};
    // mixed_*: the segments of the full-vocabulary normaliser that also exist as mixed rows (ABI 7): their indices, blocks,
    // (v_start, v_end, k, t_off, ldb) and the three scales, one entry per such segment
    JlmModel(TDict t, IDict i, FDict f, std::vector<Tensor> seg_B, std::vector<int64_t> seg_meta, std::vector<Tensor> split_B,
             std::vector<int64_t> split_meta, std::vector<double> split_t_scale, std::vector<double> split_descale,
             std::vector<int64_t> split_bias_col, std::vector<int64_t> mixed_idx, std::vector<Tensor> mixed_B,
             std::vector<int64_t> mixed_meta, std::vector<double> mixed_t_scale, std::vector<double> mixed_descale,
             std::vector<double> mixed_s8, std::vector<int64_t> mixed_head_split)
        : tensors(std::move(t)), segs(seg_B, seg_meta), split(split_B, split_meta), mixed_some(mixed_B, mixed_meta) {
        for (double x : split_t_scale) t_scale.push_back((float)x);
        for (double x : split_descale) descale.push_back((float)x);
        for (int64_t x : split_bias_col) bias_col.push_back((int)x);
        TORCH_CHECK(t_scale.size() == split.v.size() && descale.size() == split.v.size() && bias_col.size() == split.v.size(),
                    "jlm.Model: one scale / descale / bias column per split segment");
        m.segs = segs.v.data(); m.n_segs = (int)segs.v.size();
        m.b2 = tptr<const float>(tensors, "b2");
        m.H = (int)geti(i, "H"); m.ldt = (int)geti(i, "ldt");
        m.untied = (int)geti(i, "untied"); m.self_norm = (int)geti(i, "self_norm"); m.split_lstm = (int)geti(i, "split_lstm");
        m.emb = tptr<const float>(tensors, "emb"); m.ld_emb = (int)geti(i, "ld_emb");
        m.wt = tptr<const float>(tensors, "wt"); m.gate_bias = tptr<const float>(tensors, "gate_bias");
        m.kpad = (int)geti(i, "kpad"); m.E = (int)geti(i, "E");
        m.gate_descale = (float)getf(f, "gate_descale"); m.h_scale = (float)getf(f, "h_scale");
        m.wt8 = tptr<const void>(tensors, "wt8"); m.xgate8 = tptr<const float>(tensors, "xgate8");
        m.untied_split = tptr<const void>(tensors, "untied_split"); m.untied_descale = (float)getf(f, "untied_descale");
        m.lse_fixed_ref = (int)geti(i, "lse_fixed_ref");
        m.pmt = tptr<const float>(tensors, "pmt"); m.pmt_split = tptr<const void>(tensors, "pmt_split");
        m.n_t = (int)geti(i, "n_t"); m.t_descale = (float)getf(f, "t_descale");
        if (!split.v.empty()) {
            m.split_segs = split.v.data(); m.split_t_scale = t_scale.data(); m.split_descale = descale.data();
            m.split_bias_col = bias_col.data();
        }
        if (!mixed_idx.empty()) {
            const size_t n = mixed_idx.size();
            // (an untied model has no rows-stationary split table: its one segment, k = H, is checked against the f32 segment)
            TORCH_CHECK((!split.v.empty() || m.untied) && mixed_some.v.size() == n && mixed_t_scale.size() == n && mixed_descale.size() == n &&
                            mixed_s8.size() == n && (mixed_head_split.empty() || mixed_head_split.size() == n),
                        "jlm.Model: mixed segments need the split table and one block / scale / descale / s8 (/ head_split) each");
            jlm_segment none{};
            mixed.assign(segs.v.size(), none);
            mx_t_scale.assign(segs.v.size(), 0.0f); mx_descale.assign(segs.v.size(), 0.0f); mx_s8.assign(segs.v.size(), 0.0f);
            mx_head_split.assign(segs.v.size(), 0);
            for (size_t j = 0; j < n; ++j) {
                const int64_t si = mixed_idx[j];
                TORCH_CHECK(si >= 0 && si < (int64_t)segs.v.size() && !mixed[si].B, "jlm.Model: bad mixed segment index");
                const jlm_segment &a = mixed_some.v[j], &b = split.v.empty() ? segs.v[si] : split.v[si];
                TORCH_CHECK(a.v_start == b.v_start && a.v_end == b.v_end && a.k == b.k && a.t_off == b.t_off,
                            "jlm.Model: a mixed segment must describe the same words and T columns as its split form");
                TORCH_CHECK(mixed_some.keep[j].numel() >= (int64_t)(a.v_end - a.v_start) * a.ldb, "jlm.Model: mixed block too small");
                mixed[si] = a;
                mx_t_scale[si] = (float)mixed_t_scale[j]; mx_descale[si] = (float)mixed_descale[j]; mx_s8[si] = (float)mixed_s8[j];
                if (!mixed_head_split.empty()) {
                    const int64_t c = mixed_head_split[j];
                    TORCH_CHECK(c >= 0 && c % 128 == 0 && c < a.v_end - a.v_start && (c == 0 || !split.v.empty()),
                                "jlm.Model: head_split is a multiple of 128 below the segment's size, and needs the split rows");
                    mx_head_split[si] = (int)c;
                }
            }
            m.mixed_head_split = mx_head_split.data();
            m.mixed_segs = mixed.data(); m.mixed_t_scale = mx_t_scale.data(); m.mixed_descale = mx_descale.data();
            m.mixed_s8 = mx_s8.data();
            m.mixed_bias2 = tptr<const float>(tensors, "b2_log2");
        }
        TORCH_CHECK(m.b2 && m.n_segs >= 1 && m.H > 0, "jlm.Model: b2, the segments and H are required");
        TORCH_CHECK(!m.split_lstm || (m.wt8 && m.xgate8 && (m.pmt_split || m.untied)), "jlm.Model: split_lstm needs wt8, xgate8, pmt_split");
    }
};

// ------------------------------------------------------------------------------------------------- Plan
struct JlmPlan : torch::CustomClassHolder {
    TDict tensors;
    jlm_lattice lat{};
    jlm_beam_state st{};
    jlm_decode_plan p{};
    int frames_cap = 0;
    std::vector<hipEvent_t> events;         // JLM_EVENTS_PER_FRAME per frame, created on first timed decode
    int timed_frames = 0;                   // frames of the last timed decode (0: the last decode was not timed)
    int device = -1;
    int ctx_H = 0;                          // a plan with a left context: the state rows' width (0: no such plan)
    jlm_decode_cache cache{};               // the next frame loop's window (seed_cache; p.cache points here or is NULL)
    std::vector<Tensor> cache_keep;         // ... and its tensors, kept until the next seed_cache
    jlm_decode_ngram ngram{};               // the next frame loop's n-gram table (seed_ngram; p.ngram points here or is NULL)
    std::vector<Tensor> ngram_keep;         // ... and its tensors, kept until the next seed_ngram
    jlm_decode_memory memory{};             // the next frame loop's memory (seed_memory; p.memory points here or is NULL)
    std::vector<Tensor> memory_keep;        // ... and its tensors, kept until the next seed_memory

    JlmPlan(TDict t, IDict i) : tensors(std::move(t)) {
        const Tensor *ints = find(tensors, "ints");
        TORCH_CHECK(ints && ints->scalar_type() == at::kInt, "jlm.Plan: `ints` (int32 staging block) is required");
        device = ints->device().index();
        const int *base = ptr<const int>(*ints, "ints");
        auto at_off = [&](const char *key) -> const int * {
            auto it = i.find(key);
            TORCH_CHECK(it != i.end(), "jlm.Plan: missing offset ", key);
            TORCH_CHECK(it->value() >= 0 && it->value() < ints->numel(), "jlm.Plan: offset ", key, " outside `ints`");
            return base + it->value();
        };
        lat.n_sent = (int)geti(i, "n_sent"); lat.beam = (int)geti(i, "beam"); lat.n_frames = 0;
        frames_cap = (int)geti(i, "frames");
        lat.sent_len = at_off("off_sent_len"); lat.end_off = at_off("off_end_off");
        lat.node_start = at_off("off_node_start"); lat.node_word = at_off("off_node_word");
        st.score = tptr<double>(tensors, "score"); st.lse = tptr<double>(tensors, "lse"); st.ysum = tptr<double>(tensors, "ysum");
        st.bp = tptr<int>(tensors, "bp"); st.node = tptr<int>(tensors, "node"); st.word = tptr<int>(tensors, "word");
        st.cnt = tptr<int>(tensors, "cnt"); st.live = tptr<int>(tensors, "live"); st.n_live = tptr<int>(tensors, "n_live");
        st.edge = tptr<const float>(tensors, "edge"); st.live_base = tptr<int>(tensors, "live_base");
        st.lse_part = nullptr; st.ld_part = 0; st.n_parts = 0; st.flags = nullptr;
        p.kind = (int)geti(i, "kind"); p.max_cands = (int)geti(i, "max_cands");
        p.h = tptr<void>(tensors, "h"); p.c = tptr<float>(tensors, "c"); p.T = tptr<float>(tensors, "T");
        p.g0 = at_off("off_g0"); p.cidx = at_off("off_cidx"); p.sidx = at_off("off_sidx");
        p.sg_word = at_off("off_sg_word"); p.sg_off = at_off("off_sg_off"); p.sg_node = at_off("off_sg_node");
        p.edge = tptr<float>(tensors, "edge");
        p.vs_words = at_off("off_vs_words"); p.vs_off = at_off("off_vs_off");
        p.di_words = at_off("off_di_words"); p.di_off = at_off("off_di_off"); p.di_idx = at_off("off_sidx2");
        p.dd_words = at_off("off_dd_words"); p.dd_off = at_off("off_dd_off");
        // reference-compatibility lists of the incremental decoder on segmented models: present only in such plans
        p.di_wwords = i.find("off_di_wwords") != i.end() ? at_off("off_di_wwords") : nullptr;
        p.sg_wword = i.find("off_sg_wword") != i.end() ? at_off("off_sg_wword") : nullptr;
        p.run_max = tptr<float>(tensors, "run_max"); p.run_sum = tptr<double>(tensors, "run_sum");
        p.part = tptr<float>(tensors, "part"); p.max_parts = (int)geti(i, "max_parts");
        p.Tm = tptr<void>(tensors, "Tm"); p.ld_tm = (int)geti(i, "ld_tm");
        TORCH_CHECK(!p.Tm || (p.ld_tm > 0 && find(tensors, "Tm")->numel() >= (((int64_t)lat.n_sent * lat.beam + 31) / 32 * 32) * p.ld_tm),
                    "jlm.Plan: Tm must hold n_sent * beam rows (rounded up to whole 32-row blocks) of ld_tm");
        p.out_nodes = tptr<int>(tensors, "out_nodes"); p.out_len = tptr<int>(tensors, "out_len");
        p.out_score = tptr<double>(tensors, "out_score"); p.stride = (int)geti(i, "stride");
        // ABI 11: one spare element behind the trace lengths = the batch's flag word (jlm_beam_state.flags): it travels back with them
        if (p.out_len && find(tensors, "out_len")->numel() > (int64_t)lat.n_sent * lat.beam) st.flags = p.out_len + (size_t)lat.n_sent * lat.beam;
        // a plan for decodes with a left context: the root rows' prev / word (seed_context writes them) and n_sent more state rows
        p.ctx_prev = tptr<const int>(tensors, "ctx_prev"); p.ctx_word = tptr<const int>(tensors, "ctx_word");
        if (p.ctx_prev || p.ctx_word) {
            const int64_t rmax = (int64_t)lat.n_sent * lat.beam, rows = (int64_t)frames_cap * rmax + lat.n_sent, H = geti(i, "H");
            TORCH_CHECK(p.ctx_prev && p.ctx_word && find(tensors, "ctx_prev")->numel() >= rmax && find(tensors, "ctx_word")->numel() >= rmax &&
                            find(tensors, "ctx_prev")->scalar_type() == at::kInt && find(tensors, "ctx_word")->scalar_type() == at::kInt,
                        "jlm.Plan: ctx_prev and ctx_word come together, int32 [n_sent * beam]");
            TORCH_CHECK(H > 0 && p.h && p.c && find(tensors, "h")->numel() >= rows * H && find(tensors, "c")->numel() >= rows * H,
                        "jlm.Plan: a plan with a left context holds n_sent state rows behind the pool (and names H)");
            ctx_H = (int)H;
        }
        TORCH_CHECK(st.score && st.lse && st.bp && st.node && st.word && st.cnt && st.live && st.n_live && st.live_base && p.h && p.c &&
                        p.T && p.edge && p.out_nodes && p.out_len && p.out_score && lat.n_sent > 0 && lat.beam > 0 && frames_cap > 0,
                    "jlm.Plan: a required buffer is missing");
    }
    ~JlmPlan() override {
        for (hipEvent_t e : events) (void)hipEventDestroy(e);
    }
};

// side stream of each launch stream (edge logits beside the normaliser): ONE per launch stream for the whole process -- ROCm
// maps streams onto GPU_MAX_HW_QUEUES hardware queues and streams that share a queue serialise (jlm_amd/__init__.py)
std::map<std::pair<int, hipStream_t>, c10::hip::HIPStream> g_side;
// torch releases the interpreter lock around custom ops: two Python threads may be inside decode_frames at once (two
// decoders).  The side-stream table, a plan's event table and the launchers' one-time kernel
// attributes (function-local statics in libjlm_hip.so) are all touched in here: one lock around the enqueue.  It is held
// for the ~0.5 ms the launches take; the GPU work itself is asynchronous.
std::mutex g_enqueue_mutex;

int64_t decode_frames(const c10::intrusive_ptr<JlmModel> &model, const c10::intrusive_ptr<JlmPlan> &plan, int64_t n_frames,
                      int64_t vs_max, int64_t di_max, int64_t dd_max, bool use_side, bool timed, int64_t lse_cu_share_pct) {
    JlmPlan &pl = *plan;
    TORCH_CHECK(n_frames >= 1 && n_frames <= pl.frames_cap, "jlm.decode_frames: ", n_frames, " frames, the plan holds ", pl.frames_cap);
    const c10::hip::HIPGuard device_guard(pl.device);          // the plan's device, whatever the caller's current one is
    const std::lock_guard<std::mutex> lock(g_enqueue_mutex);
    c10::hip::HIPStream main = c10::hip::getCurrentHIPStream(pl.device);
    pl.lat.n_frames = (int)n_frames;
    pl.p.vs_max = (int)vs_max; pl.p.di_max = (int)di_max; pl.p.dd_max = (int)dd_max;
    pl.p.lse_cu_share_pct = (int)lse_cu_share_pct;
    void *side_s = nullptr;
    if (use_side && !timed) {
        const auto key = std::make_pair(pl.device, main.stream());
        auto it = g_side.find(key);
        if (it == g_side.end()) it = g_side.emplace(key, c10::hip::getStreamFromPool(false, pl.device)).first;
        side_s = it->second.stream();
    }
    void *const *ev = nullptr;
    pl.timed_frames = 0;
    if (timed) {
        const size_t need = (size_t)n_frames * JLM_EVENTS_PER_FRAME;
        while (pl.events.size() < need) {
            hipEvent_t e;
            jlm_check((int)hipEventCreate(&e), "hipEventCreate");
            pl.events.push_back(e);
        }
        ev = reinterpret_cast<void *const *>(pl.events.data());
        pl.timed_frames = (int)n_frames;
    }
    // (Rounds 2-4 could replay the launch sequence as a captured hipGraph, JLM_GRAPH=1: correct and slower -- 3.52-3.58 vs 2.58-2.71 ms
    //  per 256-sentence chunk, hipGraphLaunch of the 130-node two-branch graph cost more than the launches -- removed in round 5.)
    const int rc = jlm_decode_frames(&model->m, &pl.p, &pl.lat, &pl.st, main.stream(), side_s, ev);
    pl.p.cache = nullptr;                   // (seed_cache: the window of ONE frame loop)
    pl.p.ngram = nullptr;                   // (seed_ngram: the table of ONE frame loop)
    pl.p.memory = nullptr;                  // (seed_memory: the memory of ONE frame loop)
    if (rc == -2) return -2;
    jlm_check(rc, "jlm_decode_frames");
    return 0;
}

// Round 5: one batch, one op -- everything DecodeEngine._enqueue did between the staging block and the `done` event as a
// dozen torch calls (0.3-0.6 ms of interpreter time per 256-sentence chunk, tools/probes/host_profile2.py): the upload of the
// batch's lattice (head of the plan's page-locked staging block; the four node arrays straight from the lattice's own
// page-locked block), the counters' reset, the frame loop, and the read-back of the n-best traces into page-locked host
// buffers.  All asynchronous on the current stream; torch has released the interpreter lock around the whole call, so a
// second Python thread (the collector building the previous batch's strings) runs beside it.
//   host_ints [>= head_end] int32, page-locked: the staging block; blk (optional) int32, page-locked: the lattice's block, of
//   which blk_n[i] ints at blk_src[i] go to dev_ints + blk_dst[i]; without blk the whole staging block is copied.
//   h_nodes / h_len / h_score (/ h_nlive with a timed decode): page-locked destinations of out_nodes / out_len / out_score / n_live.
int64_t decode_batch(const c10::intrusive_ptr<JlmModel> &model, const c10::intrusive_ptr<JlmPlan> &plan, const Tensor &host_ints,
                     int64_t head_end, const OptTensor &blk, std::vector<int64_t> blk_src, std::vector<int64_t> blk_dst,
                     std::vector<int64_t> blk_n, const Tensor &h_nodes, const Tensor &h_len, const Tensor &h_score, const OptTensor &h_nlive,
                     int64_t n_frames, int64_t vs_max, int64_t di_max, int64_t dd_max, bool use_side, bool timed, int64_t lse_cu_share_pct) {
    JlmPlan &pl = *plan;
    const Tensor *dev_ints = find(pl.tensors, "ints");
    const Tensor *cnt = find(pl.tensors, "cnt"), *n_live = find(pl.tensors, "n_live");
    const Tensor *o_nodes = find(pl.tensors, "out_nodes"), *o_len = find(pl.tensors, "out_len"), *o_score = find(pl.tensors, "out_score");
    auto host_ok = [](const Tensor &t, at::ScalarType ty) { return t.defined() && !t.is_cuda() && t.is_contiguous() && t.scalar_type() == ty; };
    TORCH_CHECK(host_ok(host_ints, at::kInt) && host_ints.numel() <= dev_ints->numel() && head_end >= 0 && head_end <= host_ints.numel(),
                "jlm.decode_batch: the staging block must be a contiguous int32 host tensor no larger than the plan's");
    TORCH_CHECK(host_ok(h_nodes, at::kInt) && h_nodes.numel() >= o_nodes->numel() && host_ok(h_len, at::kInt) && h_len.numel() >= o_len->numel() &&
                    host_ok(h_score, at::kDouble) && h_score.numel() >= o_score->numel(),
                "jlm.decode_batch: read-back buffers");
    const bool has_blk = blk.has_value() && blk->defined();
    TORCH_CHECK(!has_blk || (host_ok(*blk, at::kInt) && blk_src.size() == blk_dst.size() && blk_src.size() == blk_n.size()), "jlm.decode_batch: lattice block");
    const c10::hip::HIPGuard device_guard(pl.device);
    hipStream_t st = c10::hip::getCurrentHIPStream(pl.device).stream();
    int *d = reinterpret_cast<int *>(dev_ints->data_ptr());
    const int *h = reinterpret_cast<const int *>(host_ints.data_ptr());
    if (!has_blk) {
        jlm_check((int)hipMemcpyAsync(d, h, (size_t)host_ints.numel() * 4, hipMemcpyHostToDevice, st), "hipMemcpyAsync (staging block)");
    } else {
        if (head_end) jlm_check((int)hipMemcpyAsync(d, h, (size_t)head_end * 4, hipMemcpyHostToDevice, st), "hipMemcpyAsync (staging head)");
        const int *b = reinterpret_cast<const int *>(blk->data_ptr());
        for (size_t i = 0; i < blk_n.size(); ++i) {
            if (blk_n[i] <= 0) continue;
            TORCH_CHECK(blk_src[i] >= 0 && blk_src[i] + blk_n[i] <= blk->numel() && blk_dst[i] >= 0 && blk_dst[i] + blk_n[i] <= dev_ints->numel(),
                        "jlm.decode_batch: a lattice array outside its block or the plan");
            jlm_check((int)hipMemcpyAsync(d + blk_dst[i], b + blk_src[i], (size_t)blk_n[i] * 4, hipMemcpyHostToDevice, st), "hipMemcpyAsync (lattice array)");
        }
    }
    jlm_check((int)hipMemsetAsync(cnt->data_ptr(), 0, (size_t)cnt->numel() * 4, st), "hipMemsetAsync (cnt)");
    jlm_check((int)hipMemsetAsync(n_live->data_ptr(), 0, (size_t)n_live->numel() * 4, st), "hipMemsetAsync (n_live)");
    if (pl.st.flags) jlm_check((int)hipMemsetAsync(pl.st.flags, 0, 4, st), "hipMemsetAsync (flags)");
    const int64_t rc = decode_frames(model, plan, n_frames, vs_max, di_max, dd_max, use_side, timed, lse_cu_share_pct);
    if (rc != 0) return rc;
    jlm_check((int)hipMemcpyAsync(h_nodes.data_ptr(), o_nodes->data_ptr(), (size_t)o_nodes->numel() * 4, hipMemcpyDeviceToHost, st), "hipMemcpyAsync (traces)");
    jlm_check((int)hipMemcpyAsync(h_len.data_ptr(), o_len->data_ptr(), (size_t)o_len->numel() * 4, hipMemcpyDeviceToHost, st), "hipMemcpyAsync (trace lengths)");
    jlm_check((int)hipMemcpyAsync(h_score.data_ptr(), o_score->data_ptr(), (size_t)o_score->numel() * 8, hipMemcpyDeviceToHost, st), "hipMemcpyAsync (scores)");
    if (h_nlive.has_value() && h_nlive->defined()) {
        TORCH_CHECK(host_ok(*h_nlive, at::kInt) && h_nlive->numel() >= n_live->numel(), "jlm.decode_batch: live-row read-back buffer");
        jlm_check((int)hipMemcpyAsync(h_nlive->data_ptr(), n_live->data_ptr(), (size_t)n_live->numel() * 4, hipMemcpyDeviceToHost, st), "hipMemcpyAsync (live rows)");
    }
    return 0;
}

// [n_frames, 5] milliseconds of the plan's last TIMED decode, which must have finished (the caller synchronised on it):
// vocab fix, lattice path fix (beam step), LSTM step, T projection + edge logits, normaliser (include/jlm_hip.h, events)
Tensor frame_times(const c10::intrusive_ptr<JlmPlan> &plan) {
    JlmPlan &pl = *plan;
    const c10::hip::HIPGuard device_guard(pl.device);
    const std::lock_guard<std::mutex> lock(g_enqueue_mutex);
    const int F = pl.timed_frames;
    Tensor out = at::zeros({F, 5}, at::kDouble);
    auto a = out.accessor<double, 2>();
    for (int f = 0; f < F; ++f) {
        const int last = (f == F - 1) ? 2 : 5;          // the last frame is not stepped
        for (int i = 0; i < last; ++i) {
            float ms = 0.0f;
            jlm_check((int)hipEventElapsedTime(&ms, pl.events[(size_t)f * JLM_EVENTS_PER_FRAME + i],
                                               pl.events[(size_t)f * JLM_EVENTS_PER_FRAME + i + 1]), "hipEventElapsedTime");
            a[f][i] = ms;
        }
    }
    return out;
}

// ------------------------------------------------------------------------------------ LSTM_Model.predict / project
void lstm_step(const Tensor &h_in, const Tensor &c_in, int64_t ld_state, const Tensor &h_out, const Tensor &c_out, const OptTensor &rows,
               const Tensor &prev, const Tensor &word, const Tensor &emb, int64_t ld_emb, const Tensor &wt, const Tensor &bias,
               int64_t kpad, int64_t H, int64_t E, int64_t n_rows_max, const OptTensor &n_dev) {
    jlm_check(jlm_lstm_step(ptr<const float>(h_in, "h_in"), ptr<const float>(c_in, "c_in"), (int)ld_state, ptr<float>(h_out, "h_out"),
                            ptr<float>(c_out, "c_out"), optr<const int>(rows, "rows"), ptr<const int>(prev, "prev"),
                            ptr<const int>(word, "word"), ptr<const float>(emb, "emb"), (int)ld_emb, ptr<const float>(wt, "wt"),
                            ptr<const float>(bias, "bias"), (int)kpad, (int)H, (int)E, (int)n_rows_max, optr<const int>(n_dev, "n_dev"),
                            stream_of(h_in)),
              "jlm_lstm_step");
}

// C[c_rows[m], n] = sum_k A[a_rows[m], k] * B[b_rows[n], k] + bias[n]; a_off / c_off / bias_off: element offsets of the
// views inside their storage (a column range of T, of the logits, of b2)
void gemm_nt(const Tensor &A, int64_t a_off, int64_t lda, const OptTensor &a_rows, const Tensor &B, int64_t ldb, const OptTensor &b_rows,
             const Tensor &C, int64_t c_off, int64_t ldc, const OptTensor &c_rows, const OptTensor &bias, int64_t bias_off, int64_t M,
             int64_t N, int64_t K, const OptTensor &m_dev) {
    TORCH_CHECK(a_off >= 0 && a_off < A.numel() && c_off >= 0 && c_off < C.numel(), "jlm.gemm_nt: offset outside the tensor");
    const float *bp = optr<const float>(bias, "bias");
    jlm_check(jlm_gemm_nt(ptr<const float>(A, "A") + a_off, (int)lda, optr<const int>(a_rows, "a_rows"), ptr<const float>(B, "B"), (int)ldb,
                          optr<const int>(b_rows, "b_rows"), ptr<float>(C, "C") + c_off, (int)ldc, optr<const int>(c_rows, "c_rows"),
                          bp ? bp + bias_off : nullptr, (int)M, (int)N, (int)K, optr<const int>(m_dev, "m_dev"), stream_of(A)),
              "jlm_gemm_nt");
}

void softmax_rows(const Tensor &y, const Tensor &pred, int64_t ld, int64_t n_rows, int64_t n_cols, bool self_norm) {
    jlm_check(jlm_softmax_rows(ptr<const float>(y, "y"), ptr<float>(pred, "pred"), (int)ld, (int)n_rows, (int)n_cols, self_norm ? 1 : 0,
                               stream_of(y)),
              "jlm_softmax_rows");
}

// ------------------------------------------------------------------------------------ weight preparation
void pack_split_f16(const Tensor &src, int64_t src_off, int64_t rows, int64_t k, int64_t ld, double scale, const Tensor &dst,
                    int64_t dst_off, int64_t ld_dst) {
    TORCH_CHECK(src_off >= 0 && src_off < src.numel() && dst_off >= 0 && dst_off < dst.numel(), "jlm.pack_split_f16: offset outside the tensor");
    jlm_check(jlm_pack_split_f16(ptr<const float>(src, "src") + src_off, (int)rows, (int)k, (int)ld, (float)scale,
                                 ptr<float>(dst, "dst") + dst_off, (int)ld_dst, stream_of(src)),
              "jlm_pack_split_f16");
}

void pack_split_f16_col(const Tensor &v, int64_t v_off, int64_t rows, double scale, const Tensor &dst, int64_t ld_dst, int64_t col) {
    TORCH_CHECK(v_off >= 0 && v_off + rows <= v.numel(), "jlm.pack_split_f16_col: range outside the vector");
    jlm_check(jlm_pack_split_f16_col(ptr<const float>(v, "v") + v_off, (int)rows, (float)scale, ptr<float>(dst, "dst"), (int)ld_dst, (int)col,
                                     stream_of(v)),
              "jlm_pack_split_f16_col");
}

// mixed rows of a vocabulary block (include/jlm_hip.h ABI 7): src [rows, k] f32 + the words' biases -> dst [rows, ld_dst]
void pack_mixed(const Tensor &src, int64_t src_off, int64_t rows, int64_t k, int64_t ld, const Tensor &bias, int64_t bias_off, double scale,
                double bias_scale, double s8, const Tensor &dst, int64_t ld_dst) {
    TORCH_CHECK(src_off >= 0 && rows >= 0 && (rows == 0 || src_off + (rows - 1) * ld + k <= src.numel()), "jlm.pack_mixed: source range");
    TORCH_CHECK(bias_off >= 0 && bias_off + rows <= bias.numel(), "jlm.pack_mixed: bias range");
    TORCH_CHECK(ld_dst % 32 == 0 && (ld_dst == (k + 2 + 31) / 32 * 32 || ld_dst == (k + 31) / 32 * 32) && rows * ld_dst <= dst.numel(),
                "jlm.pack_mixed: destination shape");
    jlm_check(jlm_pack_mixed(ptr<const float>(src, "src") + src_off, (int)rows, (int)k, (int)ld, ptr<const float>(bias, "bias") + bias_off,
                             (float)scale, (float)bias_scale, (float)s8, ptr<void>(dst, "dst"), (int)ld_dst, stream_of(src)),
              "jlm_pack_mixed");
}

// dst[r][c] = codebook[code[r][c]]: the k-means (code, codebook) form of a weight tensor expanded on the device
void dequant_u8(const Tensor &code, int64_t rows, int64_t k, int64_t ld_code, const Tensor &codebook, const Tensor &dst, int64_t ld_dst) {
    TORCH_CHECK(code.scalar_type() == at::kByte && codebook.scalar_type() == at::kFloat && dst.scalar_type() == at::kFloat,
                "jlm.dequant_u8: uint8 codes, float32 codebook and destination");
    TORCH_CHECK(rows * ld_code <= code.numel() && (rows == 0 || (rows - 1) * ld_dst + k <= dst.numel()), "jlm.dequant_u8: shape outside the tensors");
    jlm_check(jlm_dequant_u8(ptr<const uint8_t>(code, "code"), (int)rows, (int)k, (int)ld_code, ptr<const float>(codebook, "codebook"),
                             (int)codebook.numel(), ptr<float>(dst, "dst"), (int)ld_dst, stream_of(code)),
              "jlm_dequant_u8");
}

// the normaliser slices of a few probe rows in one of its forms (jlm_lse_probe, include/jlm_hip.h ABI 8): -> number of slices, -2
// when the model has no such form
int64_t lse_probe(const c10::intrusive_ptr<JlmModel> &model, const Tensor &rowlist, const Tensor &prev, const Tensor &word, int64_t steps,
                  int64_t rows, const Tensor &h, const Tensor &c, const Tensor &T, const OptTensor &Tm, int64_t ld_tm, int64_t form,
                  const Tensor &part, int64_t max_parts) {
    const int64_t G = (steps + 1) * rows;
    TORCH_CHECK(steps >= 1 && rows >= 1 && rowlist.numel() >= G && prev.numel() >= G && word.numel() >= G, "jlm.lse_probe: index arrays");
    TORCH_CHECK(rowlist.scalar_type() == at::kInt && prev.scalar_type() == at::kInt && word.scalar_type() == at::kInt, "jlm.lse_probe: int32 indices");
    TORCH_CHECK(h.numel() >= G * model->m.H && c.numel() >= G * model->m.H && T.numel() >= G * model->m.ldt, "jlm.lse_probe: state buffers");
    TORCH_CHECK(part.numel() >= max_parts * rows * 2 && max_parts >= 1, "jlm.lse_probe: slice buffer");
    TORCH_CHECK(!Tm.has_value() || !Tm->defined() || Tm->numel() >= ((rows + 31) / 32 * 32) * ld_tm, "jlm.lse_probe: packed-row buffer (whole 32-row blocks)");
    const c10::hip::HIPGuard device_guard(h.device().index());
    const std::lock_guard<std::mutex> lock(g_enqueue_mutex);
    const int rc = jlm_lse_probe(&model->m, ptr<const int>(rowlist, "rowlist"), ptr<const int>(prev, "prev"), ptr<const int>(word, "word"),
                                 (int)steps, (int)rows, ptr<void>(h, "h"), ptr<float>(c, "c"), ptr<float>(T, "T"), optr<void>(Tm, "Tm"),
                                 (int)ld_tm, (int)form, ptr<float>(part, "part"), (int)max_parts, stream_of(h));
    if (rc == -2 || rc >= 1) return rc;
    jlm_check(rc == 0 ? -1 : rc, "jlm_lse_probe");
    return rc;
}

// The checks the row-set frame ops share (score_frames, generate_frames, complete_frames): n_live_host holds n_counts live-row
// counts, one per `unit`, each in [0, max_live]; h0 / c0 and h1 / c1 are the two ping-pong state row sets of n_rows rows of H 4-byte
// values (c: float32).
void check_row_sets(const char *op, const jlm_decode_model &m, int64_t n_rows, const Tensor &h0, const Tensor &c0, const Tensor &h1,
                    const Tensor &c1, const std::vector<int64_t> &n_live_host, int64_t n_counts, const char *unit, int64_t max_live) {
    const int64_t R = n_rows;
    auto is_f32 = [](const Tensor &t, int64_t n) { return t.defined() && t.scalar_type() == at::kFloat && t.numel() >= n; };
    TORCH_CHECK(R >= 0 && n_counts >= 0 && (int64_t)n_live_host.size() == n_counts, "jlm.", op, ": n_live_host holds one count per ", unit);
    for (int64_t x : n_live_host) TORCH_CHECK(x >= 0 && x <= max_live, "jlm.", op, ": a live-row count outside [0, ", max_live, "]");
    TORCH_CHECK(h0.numel() >= R * m.H && h1.numel() >= R * m.H && h0.element_size() == 4 && h1.element_size() == 4 &&
                    is_f32(c0, R * m.H) && is_f32(c1, R * m.H),
                "jlm.", op, ": state row sets [", R, ", H] of 4-byte values");
}

// Enqueue one frame op, launch(stream, events), on the current stream of device `dev` under the enqueue lock.  Timed: with
// n_frames x per_frame events, and -> [n_frames, per_frame - 1] milliseconds between each frame's consecutive events after waiting
// for the last.  Untimed, or with no frame recorded (n_frames = 0): an empty tensor, and nothing waits.
template <class Launch>
Tensor launch_frames(const char *what, int dev, bool timed, int64_t n_frames, int per_frame, Launch launch) {
    const c10::hip::HIPGuard device_guard(dev);
    hipStream_t st = c10::hip::getCurrentHIPStream(dev).stream();
    std::vector<hipEvent_t> ev;
    struct Destroy {
        std::vector<hipEvent_t> &ev;
        ~Destroy() { for (hipEvent_t e : ev) (void)hipEventDestroy(e); }
    } destroy{ev};
    if (timed)
        for (int64_t i = 0; i < n_frames * per_frame; ++i) {
            hipEvent_t e;
            jlm_check((int)hipEventCreate(&e), "hipEventCreate");
            ev.push_back(e);
        }
    {
        const std::lock_guard<std::mutex> lock(g_enqueue_mutex);
        jlm_check(launch(st, timed ? reinterpret_cast<void *const *>(ev.data()) : nullptr), what);
    }
    if (!timed || n_frames == 0) return at::empty({0}, at::kDouble);
    jlm_check((int)hipEventSynchronize(ev.back()), "hipEventSynchronize");
    Tensor out = at::zeros({n_frames, per_frame - 1}, at::kDouble);
    auto a = out.accessor<double, 2>();
    for (int64_t f = 0; f < n_frames; ++f)
        for (int i = 0; i + 1 < per_frame; ++i) {
            float ms = 0.0f;
            jlm_check((int)hipEventElapsedTime(&ms, ev[f * per_frame + i], ev[f * per_frame + i + 1]), "hipEventElapsedTime");
            a[f][i] = ms;
        }
    return out;
}

// The state a decode with a left context starts from (jlm_prime_frames, include/jlm_hip.h): n_steps LSTM steps over right-aligned word
// rows, nothing else.  State row sets h0/c0 and h1/c1, ping-pong (the result is in set n_steps % 2); rows [n_rows], prev / word
// [n_steps][n_rows], n_live [n_steps] int32 and its host copy.  Every id must lie in [0, V): the caller checks (jlm_amd/context.py).
void prime_frames(const c10::intrusive_ptr<JlmModel> &model, const Tensor &h0, const Tensor &c0, const Tensor &h1, const Tensor &c1,
                  const Tensor &rows, const Tensor &prev, const Tensor &word, const Tensor &n_live, std::vector<int64_t> n_live_host,
                  int64_t n_rows, int64_t n_steps) {
    const jlm_decode_model &m = model->m;
    const int64_t R = n_rows, S = n_steps;
    check_row_sets("prime_frames", m, R, h0, c0, h1, c1, n_live_host, S, "frame", R);
    TORCH_CHECK(is(rows, at::kInt, R) && is(prev, at::kInt, S * R) && is(word, at::kInt, S * R) && is(n_live, at::kInt, S),
                "jlm.prime_frames: int32 rows [n_rows], prev / word [n_steps][n_rows], n_live [n_steps]");
    TORCH_CHECK(R * (int64_t)std::max(m.H / 4, 1) < 0x7ffffff0ll, "jlm.prime_frames: rows x H / 4 must stay below 2^31");
    jlm_prime_plan p{};
    p.n_rows = (int)R; p.n_steps = (int)S;
    p.h[0] = ptr<void>(h0, "h0"); p.h[1] = ptr<void>(h1, "h1"); p.c[0] = ptr<float>(c0, "c0"); p.c[1] = ptr<float>(c1, "c1");
    p.rows = ptr<const int>(rows, "rows"); p.prev = ptr<const int>(prev, "prev"); p.word = ptr<const int>(word, "word");
    p.n_live = ptr<const int>(n_live, "n_live");
    std::vector<int> live_host(n_live_host.begin(), n_live_host.end());
    p.n_live_host = live_host.data();
    (void)launch_frames("jlm_prime_frames", h0.device().index(), false, 0, 1,
                        [&](hipStream_t st, void *const *) { return jlm_prime_frames(&m, &p, st); });
}

// The primed states of a batch's sentences gathered behind the plan's state pool, and the root rows' prev / word (jlm_seed_context):
// one launch on the current stream, in front of the plan's frame loop.  src_h / src_c [n_src, H] in the model's state-row format,
// last / has [n_src] int32, idx [n_sent] int32 on the device (the caller keeps 0 <= idx < n_src).
void seed_context(const c10::intrusive_ptr<JlmPlan> &plan, const Tensor &src_h, const Tensor &src_c, const Tensor &last, const Tensor &has,
                  const Tensor &idx) {
    JlmPlan &pl = *plan;
    TORCH_CHECK(pl.ctx_H > 0 && pl.p.ctx_prev && pl.p.ctx_word, "jlm.seed_context: the plan was made without ctx_prev / ctx_word");
    const int64_t H = pl.ctx_H, n_src = last.numel();
    TORCH_CHECK(src_h.defined() && src_h.element_size() == 4 && src_h.numel() >= n_src * H && is(src_c, at::kFloat, n_src * H) &&
                    is(last, at::kInt, n_src) && is(has, at::kInt, n_src) && is(idx, at::kInt, pl.lat.n_sent),
                "jlm.seed_context: src_h / src_c [n_src, H] of 4-byte values, int32 last / has [n_src], idx [n_sent]");
    const c10::hip::HIPGuard device_guard(pl.device);
    const long long G = (long long)pl.frames_cap * pl.lat.n_sent * pl.lat.beam;
    jlm_check(jlm_seed_context(ptr<const void>(src_h, "src_h"), ptr<const float>(src_c, "src_c"), (int)H, ptr<const int>(last, "last"),
                               ptr<const int>(has, "has"), (int)n_src, ptr<const int>(idx, "idx"), pl.lat.n_sent, pl.lat.beam, G, pl.p.h,
                               pl.p.c, const_cast<int *>(pl.p.ctx_prev), const_cast<int *>(pl.p.ctx_word),
                               c10::hip::getCurrentHIPStream(pl.device).stream()),
              "jlm_seed_context");
}

// prime_frames that keeps its states (jlm_prime_cache_frames): target [n_steps][n_rows] int32, and the window's hist [cap][n_rows][H]
// (4-byte values) / words [cap][n_rows] int32, which take the last `cap` frames' live rows and targets.
void prime_cache_frames(const c10::intrusive_ptr<JlmModel> &model, const Tensor &h0, const Tensor &c0, const Tensor &h1, const Tensor &c1,
                        const Tensor &rows, const Tensor &prev, const Tensor &word, const Tensor &n_live, std::vector<int64_t> n_live_host,
                        int64_t n_rows, int64_t n_steps, const Tensor &target, const Tensor &hist, const Tensor &words, int64_t cap) {
    const jlm_decode_model &m = model->m;
    const int64_t R = n_rows, S = n_steps;
    check_row_sets("prime_cache_frames", m, R, h0, c0, h1, c1, n_live_host, S, "frame", R);
    TORCH_CHECK(is(rows, at::kInt, R) && is(prev, at::kInt, S * R) && is(word, at::kInt, S * R) && is(n_live, at::kInt, S) &&
                    is(target, at::kInt, S * R),
                "jlm.prime_cache_frames: int32 rows [n_rows], prev / word / target [n_steps][n_rows], n_live [n_steps]");
    TORCH_CHECK(cap >= 1 && cap <= 0x7fffffff / std::max<int64_t>(R, 1) && hist.defined() && hist.is_cuda() && hist.is_contiguous() &&
                    hist.element_size() == 4 && hist.numel() >= cap * R * m.H && is(words, at::kInt, cap * R),
                "jlm.prime_cache_frames: hist [cap][n_rows][H] of 4-byte values, int32 words [cap][n_rows]");
    TORCH_CHECK(R * (int64_t)std::max(m.H / 4, 1) < 0x7ffffff0ll, "jlm.prime_cache_frames: rows x H / 4 must stay below 2^31");
    jlm_prime_plan p{};
    p.n_rows = (int)R; p.n_steps = (int)S;
    p.h[0] = ptr<void>(h0, "h0"); p.h[1] = ptr<void>(h1, "h1"); p.c[0] = ptr<float>(c0, "c0"); p.c[1] = ptr<float>(c1, "c1");
    p.rows = ptr<const int>(rows, "rows"); p.prev = ptr<const int>(prev, "prev"); p.word = ptr<const int>(word, "word");
    p.n_live = ptr<const int>(n_live, "n_live");
    std::vector<int> live_host(n_live_host.begin(), n_live_host.end());
    p.n_live_host = live_host.data();
    (void)launch_frames("jlm_prime_cache_frames", h0.device().index(), false, 0, 1, [&](hipStream_t st, void *const *) {
        return jlm_prime_cache_frames(&m, &p, ptr<const int>(target, "target"), hist.data_ptr(), ptr<int>(words, "words"), (int)cap, st);
    });
}

// The window of a batch's sentences for the plan's NEXT frame loop (jlm_decode_plan.cache): no launch, the plan keeps the tensors.
// hist [cap][n_src][H] (4-byte values), words [cap][n_src], count [n_src], idx [n_sent] int32 on the device, the scratch s
// [n_sent * beam][ld_s] float32.  The frame loop that follows takes the struct and clears it: a later batch starts without a cache.
void seed_cache(const c10::intrusive_ptr<JlmPlan> &plan, const Tensor &hist, const Tensor &words, const Tensor &count, const Tensor &idx,
                const Tensor &s, int64_t cap, int64_t N, double theta, double lam) {
    JlmPlan &pl = *plan;
    const int64_t n_src = count.numel(), rmax = (int64_t)pl.lat.n_sent * pl.lat.beam;
    TORCH_CHECK(pl.ctx_H > 0, "jlm.seed_cache: the plan was made without a left context");
    TORCH_CHECK(cap >= 1 && N >= 1 && N <= JLM_CACHE_MIX_MAX_N && n_src >= 1 && n_src <= 0x7fffffff / cap, "jlm.seed_cache: cap, N or the row count");
    const int64_t ld_s = rmax > 0 ? s.numel() / rmax : 0;
    TORCH_CHECK(hist.defined() && hist.is_cuda() && hist.is_contiguous() && hist.element_size() == 4 && hist.numel() >= cap * n_src * pl.ctx_H &&
                    is(words, at::kInt, cap * n_src) && is(count, at::kInt, n_src) && is(idx, at::kInt, pl.lat.n_sent) &&
                    is(s, at::kFloat, rmax * std::min(cap, N)) && ld_s >= std::min(cap, N),
                "jlm.seed_cache: hist [cap][n_src][H], int32 words [cap][n_src], count [n_src], idx [n_sent], float32 s [n_sent * beam][>= min(cap, N)]");
    TORCH_CHECK(theta >= 0.0 && theta < 3.0e38 && lam > 0.0 && lam < 1.0, "jlm.seed_cache: theta >= 0, 0 < lam < 1");
    pl.cache_keep = {hist, words, count, idx, s};
    pl.cache.hist = hist.data_ptr(); pl.cache.words = ptr<const int>(words, "words"); pl.cache.count = ptr<const int>(count, "count");
    pl.cache.cap = (int)cap; pl.cache.n_src = (int)n_src; pl.cache.idx = ptr<const int>(idx, "idx");
    pl.cache.N = (int)N; pl.cache.theta = (float)theta; pl.cache.lam = (float)lam;
    pl.cache.s = ptr<float>(s, "s"); pl.cache.ld_s = (int)ld_s;
    pl.p.cache = &pl.cache;
}

// seed_cache undone: a batch that failed between seed_cache and its frame loop leaves no window behind on the plan
void clear_cache(const c10::intrusive_ptr<JlmPlan> &plan) {
    plan->p.cache = nullptr;
    plan->cache_keep.clear();
}

// The n-gram table of the plan's NEXT frame loop (jlm_decode_plan.ngram): no launch, the plan keeps the tensors.  keys [2^log2cap] int64
// (the table's 64-bit keys, bit for bit), vals [2^log2cap][2] float32, root_hist [n_sent][2] int32 on the device.  The frame loop that
// follows takes the struct and clears it: a later batch starts without a table.
void seed_ngram(const c10::intrusive_ptr<JlmPlan> &plan, const Tensor &keys, const Tensor &vals, const Tensor &root_hist, int64_t log2cap,
                int64_t max_probe, int64_t order, double lam) {
    JlmPlan &pl = *plan;
    TORCH_CHECK(log2cap >= 6 && log2cap <= 31 && max_probe >= 0 && max_probe < ((int64_t)1 << log2cap) && order >= 1 && order <= 3,
                "jlm.seed_ngram: log2cap 6 .. 31, 0 <= max_probe < 2^log2cap, order 1 .. 3");
    const int64_t cap = (int64_t)1 << log2cap;
    TORCH_CHECK(is(keys, at::kLong, cap) && keys.numel() == cap && is(vals, at::kFloat, 2 * cap) && vals.numel() == 2 * cap &&
                    is(root_hist, at::kInt, 2 * (int64_t)pl.lat.n_sent) && keys.is_cuda() && vals.is_cuda() && root_hist.is_cuda() &&
                    keys.is_contiguous() && vals.is_contiguous() && root_hist.is_contiguous() &&
                    keys.device().index() == pl.device && vals.device().index() == pl.device && root_hist.device().index() == pl.device,
                "jlm.seed_ngram: int64 keys [2^log2cap], float32 vals [2^log2cap][2], int32 root_hist [n_sent][2] on the plan's device");
    TORCH_CHECK(lam > 0.0 && lam < 1.0 && (float)lam > 0.0f && (float)lam < 1.0f, "jlm.seed_ngram: 0 < lam < 1");
    pl.ngram_keep = {keys, vals, root_hist};
    pl.ngram.keys = keys.data_ptr(); pl.ngram.vals = ptr<const float>(vals, "vals");
    pl.ngram.log2cap = (int)log2cap; pl.ngram.max_probe = (int)max_probe; pl.ngram.order = (int)order; pl.ngram.lam = (float)lam;
    pl.ngram.root_hist = ptr<const int>(root_hist, "root_hist");
    pl.p.ngram = &pl.ngram;
}

// seed_ngram undone: a batch that failed between seed_ngram and its frame loop leaves no table behind on the plan
void clear_ngram(const c10::intrusive_ptr<JlmPlan> &plan) {
    plan->p.ngram = nullptr;
    plan->ngram_keep.clear();
}

// The memory of the plan's NEXT frame loop (jlm_decode_plan.memory): no launch, the plan keeps the tensors.  keys [N][H] (4-byte values,
// the model's state-row format), key_words [N] int32; the buffers of one frame's retrieval over the plan's n_sent * beam rows: q_rows
// [rows][H] float32, s [rows][ld_s >= K] float32, ret_words [K][rows] int32, the workspace (float32, jlm_memory_topk's) and one int32 of
// flags.  The frame loop that follows takes the struct and clears it: a later batch starts without a memory.  Unlike seed_cache, any
// plan will do: a left context is not needed.
void seed_memory(const c10::intrusive_ptr<JlmPlan> &plan, const Tensor &keys, const Tensor &key_words, int64_t N, int64_t H, double theta,
                 double lam, int64_t K, const Tensor &q_rows, const Tensor &s, const Tensor &ret_words, const Tensor &workspace,
                 const Tensor &flags) {
    JlmPlan &pl = *plan;
    const int64_t rmax = (int64_t)pl.lat.n_sent * pl.lat.beam;
    TORCH_CHECK(N >= 1 && N <= 0x7fffffff && H >= 4 && H % 4 == 0 && K >= 1 && K <= JLM_MEMORY_TOPK_MAX && rmax >= 1 && rmax <= 65535,
                "jlm.seed_memory: N >= 1, H % 4 == 0, 1 <= K <= ", JLM_MEMORY_TOPK_MAX, ", at most 65535 rows a batch");
    const int64_t ld_s = s.defined() ? s.numel() / rmax : 0;
    auto on_dev = [&](const Tensor &t) { return t.defined() && t.is_cuda() && t.is_contiguous() && t.device().index() == pl.device; };
    TORCH_CHECK(on_dev(keys) && keys.element_size() == 4 && keys.numel() >= N * H && on_dev(key_words) && is(key_words, at::kInt, N) &&
                    on_dev(q_rows) && is(q_rows, at::kFloat, rmax * H) && on_dev(s) && is(s, at::kFloat, rmax * K) && ld_s >= K &&
                    on_dev(ret_words) && is(ret_words, at::kInt, K * rmax) && on_dev(workspace) && is(workspace, at::kFloat, 1) &&
                    on_dev(flags) && is(flags, at::kInt, 1),
                "jlm.seed_memory: keys [N][H], int32 key_words [N], float32 q_rows [rows][H], s [rows][>= K], int32 ret_words [K][rows], "
                "a float32 workspace and int32 flags [1] on the plan's device");
    TORCH_CHECK(theta >= 0.0 && theta < 3.0e38 && lam > 0.0 && lam < 1.0 && (float)lam > 0.0f && (float)lam < 1.0f,
                "jlm.seed_memory: theta >= 0, 0 < lam < 1");
    pl.memory_keep = {keys, key_words, q_rows, s, ret_words, workspace, flags};
    pl.memory.keys = keys.data_ptr(); pl.memory.key_words = ptr<const int>(key_words, "key_words");
    pl.memory.N = (int)N; pl.memory.K = (int)K; pl.memory.theta = (float)theta; pl.memory.lam = (float)lam;
    pl.memory.q_rows = q_rows.data_ptr(); pl.memory.s = ptr<float>(s, "s"); pl.memory.ld_s = (int)ld_s;
    pl.memory.ret_words = ptr<int>(ret_words, "ret_words");
    pl.memory.workspace = workspace.data_ptr(); pl.memory.workspace_bytes = (size_t)workspace.numel() * 4;
    pl.memory.flags = ptr<int>(flags, "flags");
    pl.p.memory = &pl.memory;
}

// seed_memory undone: a batch that failed between seed_memory and its frame loop leaves no memory behind on the plan
void clear_memory(const c10::intrusive_ptr<JlmPlan> &plan) {
    plan->p.memory = nullptr;
    plan->memory_keep.clear();
}

// The predictions of an unfinished last word behind a plan's static decode (jlm_tail_predict): one launch on the current stream, which
// must be the one the plan's decode_frames / decode_batch ran on -- it reads that decode's pools.  ids [n_ids] int32: the vocabulary
// sorted by (reading, id); sp_off [n_sent + 1], sp_frame / sp_lo / sp_hi [n_spans] int32: the batch's spans; out_score [n_sent * n_out]
// f64, out_row / out_word / out_len [n_sent * n_out] int32, out_nodes [n_sent * n_out, stride] int32.  chunk 0: the launcher's default.
void tail_predict(const c10::intrusive_ptr<JlmModel> &model, const c10::intrusive_ptr<JlmPlan> &plan, const Tensor &ids, const Tensor &sp_off,
                  const Tensor &sp_frame, const Tensor &sp_lo, const Tensor &sp_hi, int64_t n_out, int64_t chunk, const Tensor &out_score,
                  const Tensor &out_row, const Tensor &out_word, const Tensor &out_nodes, const Tensor &out_len, int64_t stride) {
    JlmPlan &pl = *plan;
    const jlm_decode_model &m = model->m;
    const int64_t B = pl.lat.n_sent, R = B * n_out;
    TORCH_CHECK(pl.p.kind != 2 && pl.lat.n_frames >= 1, "jlm.tail_predict: the plan must have run a static decode");
    TORCH_CHECK(n_out >= 1 && n_out <= 64 && stride >= 1 && chunk >= 0 && chunk <= (1 << 20), "jlm.tail_predict: n_out is 1 .. 64, stride >= 1, chunk >= 0");
    TORCH_CHECK(is(ids, at::kInt, 1) && is(sp_off, at::kInt, B + 1) && sp_frame.defined() && is(sp_lo, at::kInt, sp_frame.numel()) &&
                    is(sp_hi, at::kInt, sp_frame.numel()) && sp_frame.scalar_type() == at::kInt && sp_frame.numel() >= 1,
                "jlm.tail_predict: int32 ids, sp_off [n_sent + 1], sp_frame / sp_lo / sp_hi of one length");
    TORCH_CHECK(is(out_score, at::kDouble, R) && is(out_row, at::kInt, R) && is(out_word, at::kInt, R) && is(out_len, at::kInt, R) &&
                    is(out_nodes, at::kInt, R * stride),
                "jlm.tail_predict: outputs of n_sent * n_out entries (out_nodes: x stride)");
    const c10::hip::HIPGuard device_guard(pl.device);
    const std::lock_guard<std::mutex> lock(g_enqueue_mutex);          // (the launcher's one-time kernel attribute)
    jlm_check(jlm_tail_predict(m.segs, m.n_segs, m.b2, pl.p.T, m.ldt, pl.lat.n_sent, pl.lat.beam, pl.lat.n_frames, pl.st.score, pl.st.lse,
                               pl.st.cnt, pl.st.bp, pl.st.node, m.self_norm ? 1 : 0, ptr<const int>(ids, "ids"), (int)ids.numel(),
                               ptr<const int>(sp_off, "sp_off"), ptr<const int>(sp_frame, "sp_frame"), ptr<const int>(sp_lo, "sp_lo"),
                               ptr<const int>(sp_hi, "sp_hi"), (int)n_out, (int)chunk, ptr<double>(out_score, "out_score"),
                               ptr<int>(out_row, "out_row"), ptr<int>(out_word, "out_word"), ptr<int>(out_nodes, "out_nodes"),
                               ptr<int>(out_len, "out_len"), (int)stride, c10::hip::getCurrentHIPStream(pl.device).stream()),
              "jlm_tail_predict");
}

// teacher-forced scoring of n_rows sequences / streams over n_steps steps (jlm_score_frames, include/jlm_hip.h): state row sets h0/c0
// (read by step 0) and h1/c1, ping-pong; T / Tm / part as the model's normaliser needs them; word / target [n_steps][n_rows] int32;
// n_live [n_steps] int32 on the device and its host copy; nll_seq [n_rows] f64 (accumulated), nll_tok [n_steps][n_rows] f64 (optional),
// flags one int32 (optional).  Every id must lie in [0, V): the caller checks (jlm_amd/score.py) -- the kernels index with them.
// -> timed: [n_steps, 4] milliseconds per step (LSTM step, T projection, normaliser, fold) after waiting for the last step; else an
// empty tensor and nothing waits.
// (the checked "forced rows" of a teacher-forced plan, jlm_score_plan or jlm_rank_plan: the state row sets, T, rows / prev0, word / target
//  and n_live; live_host keeps the plan's host counts alive)
template <class Plan> struct ForcedPlanArgs {
    Plan p{};
    std::vector<int> live_host;
    ForcedPlanArgs(const char *op, const jlm_decode_model &m, const Tensor &h0, const Tensor &c0, const Tensor &h1, const Tensor &c1,
                   const OptTensor &T, const Tensor &rows, const Tensor &prev0, const Tensor &word, const Tensor &target, const Tensor &n_live,
                   const std::vector<int64_t> &n_live_host, int64_t R, int64_t S)
        : live_host(n_live_host.begin(), n_live_host.end()) {
        check_row_sets(op, m, R, h0, c0, h1, c1, n_live_host, S, "step", R);
        TORCH_CHECK(is(rows, at::kInt, R) && is(prev0, at::kInt, R) && is(word, at::kInt, S * R) && is(target, at::kInt, S * R) &&
                        is(n_live, at::kInt, S),
                    "jlm.", op, ": int32 rows / prev0 [n_rows], word / target [n_steps][n_rows], n_live [n_steps]");
        TORCH_CHECK(!has(T) || is(*T, at::kFloat, R * m.ldt), "jlm.", op, ": T [n_rows, ldt] float32");
        p.n_rows = (int)R; p.n_steps = (int)S;
        p.h[0] = ptr<void>(h0, "h0"); p.h[1] = ptr<void>(h1, "h1"); p.c[0] = ptr<float>(c0, "c0"); p.c[1] = ptr<float>(c1, "c1");
        p.T = optr<float>(T, "T");
        p.rows = ptr<const int>(rows, "rows"); p.prev0 = ptr<const int>(prev0, "prev0");
        p.word = ptr<const int>(word, "word"); p.target = ptr<const int>(target, "target"); p.n_live = ptr<const int>(n_live, "n_live");
        p.n_live_host = live_host.data();
    }
};

// (the checked jlm_score_plan of score_frames and score_cache_frames)
struct ScorePlanArgs : ForcedPlanArgs<jlm_score_plan> {
    ScorePlanArgs(const char *op, const jlm_decode_model &m, const Tensor &h0, const Tensor &c0, const Tensor &h1, const Tensor &c1,
                  const OptTensor &T, const OptTensor &Tm, int64_t ld_tm, const OptTensor &part, int64_t max_parts, const Tensor &rows,
                  const Tensor &prev0, const Tensor &word, const Tensor &target, const Tensor &n_live, const std::vector<int64_t> &n_live_host,
                  const Tensor &nll_seq, const OptTensor &nll_tok, const OptTensor &flags, int64_t R, int64_t S)
        : ForcedPlanArgs(op, m, h0, c0, h1, c1, T, rows, prev0, word, target, n_live, n_live_host, R, S) {
        TORCH_CHECK(is(nll_seq, at::kDouble, R) && opt_ok(nll_tok, at::kDouble, S * R) && opt_ok(flags, at::kInt, 1),
                    "jlm.", op, ": float64 nll_seq [n_rows] / nll_tok [n_steps][n_rows], int32 flags");
        TORCH_CHECK(!has(part) || (is(*part, at::kFloat, max_parts * R * 2) && max_parts >= 1), "jlm.", op, ": part [max_parts][n_rows][2]");
        TORCH_CHECK(!has(Tm) || (ld_tm > 0 && Tm->numel() >= ((R + 31) / 32 * 32) * ld_tm), "jlm.", op, ": Tm (whole 32-row blocks of ld_tm)");
        p.Tm = optr<void>(Tm, "Tm"); p.ld_tm = p.Tm ? (int)ld_tm : 0;
        p.part = optr<float>(part, "part"); p.max_parts = p.part ? (int)max_parts : 0;
        p.nll_seq = ptr<double>(nll_seq, "nll_seq"); p.nll_tok = optr<double>(nll_tok, "nll_tok"); p.flags = optr<int>(flags, "flags");
    }
};

Tensor score_frames(const c10::intrusive_ptr<JlmModel> &model, const Tensor &h0, const Tensor &c0, const Tensor &h1, const Tensor &c1,
                    const OptTensor &T, const OptTensor &Tm, int64_t ld_tm, const OptTensor &part, int64_t max_parts, const Tensor &rows,
                    const Tensor &prev0, const Tensor &word, const Tensor &target, const Tensor &n_live, std::vector<int64_t> n_live_host,
                    const Tensor &nll_seq, const OptTensor &nll_tok, const OptTensor &flags, int64_t n_rows, int64_t n_steps, bool timed) {
    const jlm_decode_model &m = model->m;
    const int64_t R = n_rows, S = n_steps;
    const ScorePlanArgs sp("score_frames", m, h0, c0, h1, c1, T, Tm, ld_tm, part, max_parts, rows, prev0, word, target, n_live, n_live_host,
                           nll_seq, nll_tok, flags, R, S);
    return launch_frames("jlm_score_frames", h0.device().index(), timed, R > 0 ? S : 0, JLM_SCORE_EVENTS_PER_STEP,
                         [&](hipStream_t st, void *const *ev) { return jlm_score_frames(&m, &sp.p, st, ev); });
}

// The per-segment candidate lists behind a plan's static decode (jlm_alt_frames, include/jlm_hip.h): alt_head_kernel over the plan's
// pools, then score_frames' launches over the same rows, on the current stream.  The plan's decode must have COMPLETED (the caller has
// waited for its ticket's event: DecodeEngine.collect) and the plan must still be held; the stream need not be the decode's.
// rank: the path; sent_off [n_sent + 1], sent_rows / depth / alt [n_rows] int32 on the device; the rest are score_frames' arguments
// (prev0 and nll_seq are written by the head launch: the caller zeroes nothing).  -> as score_frames.
Tensor alt_frames(const c10::intrusive_ptr<JlmModel> &model, const c10::intrusive_ptr<JlmPlan> &plan, int64_t rank, const Tensor &sent_off,
                  const Tensor &sent_rows, const Tensor &depth, const Tensor &alt, const Tensor &h0, const Tensor &c0, const Tensor &h1,
                  const Tensor &c1, const OptTensor &T, const OptTensor &Tm, int64_t ld_tm, const OptTensor &part, int64_t max_parts,
                  const Tensor &rows, const Tensor &prev0, const Tensor &word, const Tensor &target, const Tensor &n_live,
                  std::vector<int64_t> n_live_host, const Tensor &nll_seq, const OptTensor &nll_tok, const OptTensor &flags, int64_t n_rows,
                  int64_t n_steps, bool timed) {
    JlmPlan &pl = *plan;
    const jlm_decode_model &m = model->m;
    const int64_t R = n_rows, S = n_steps, B = pl.lat.n_sent;
    TORCH_CHECK(pl.p.kind == 0 && pl.lat.n_frames >= 1, "jlm.alt_frames: the plan must have run a static full-vocabulary decode");
    TORCH_CHECK(rank >= 0 && rank < pl.lat.beam, "jlm.alt_frames: rank is 0 .. beam - 1");
    TORCH_CHECK(is(sent_off, at::kInt, B + 1) && is(sent_rows, at::kInt, R) && is(depth, at::kInt, R) && is(alt, at::kInt, R),
                "jlm.alt_frames: int32 sent_off [n_sent + 1], sent_rows / depth / alt [n_rows]");
    TORCH_CHECK(h0.device().index() == pl.device, "jlm.alt_frames: the row sets live on the plan's device");
    TORCH_CHECK(R * (int64_t)std::max(m.H / 4, 1) < 0x7ffffff0ll, "jlm.alt_frames: rows x H / 4 must stay below 2^31");
    const ScorePlanArgs sp("alt_frames", m, h0, c0, h1, c1, T, Tm, ld_tm, part, max_parts, rows, prev0, word, target, n_live, n_live_host,
                           nll_seq, nll_tok, flags, R, S);
    jlm_alt_plan a{};
    a.n_sent = pl.lat.n_sent; a.beam = pl.lat.beam; a.n_frames = pl.lat.n_frames; a.rank = (int)rank;
    a.h = pl.p.h; a.c = pl.p.c; a.T = pl.p.T; a.score = pl.st.score; a.lse = pl.st.lse; a.bp = pl.st.bp; a.sent_len = pl.lat.sent_len;
    a.sent_off = ptr<const int>(sent_off, "sent_off"); a.sent_rows = ptr<const int>(sent_rows, "sent_rows");
    a.depth = ptr<const int>(depth, "depth"); a.alt = ptr<const int>(alt, "alt"); a.prev0 = ptr<int>(prev0, "prev0");
    jlm_check(jlm_alt_head_refuse(m.segs, m.n_segs, m.b2, m.ldt, m.H, m.self_norm ? 1 : 0, &a, &sp.p), "jlm_alt_frames");
    return launch_frames("jlm_alt_frames", pl.device, timed, R > 0 ? S : 0, JLM_SCORE_EVENTS_PER_STEP,
                         [&](hipStream_t st, void *const *ev) { return jlm_alt_frames(&m, &a, &sp.p, st, ev); });
}

// The ring of a cache op, checked, into its plan (jlm_cache_plan, jlm_cache_mix_plan, jlm_predict_cache_plan): hist, words, cap and N; the
// caller has checked its own bounds on cap and its position.
template <class Plan>
void ring_into(const char *op, Plan &cp, int64_t H, int64_t R, const Tensor &hist, const Tensor &words, int64_t cap, int64_t N) {
    TORCH_CHECK(hist.defined() && hist.element_size() == 4 && hist.numel() >= cap * R * H && is(words, at::kInt, cap * R),
                "jlm.", op, ": hist [cap][n_rows][H] of 4-byte values, int32 words [cap][n_rows]");
    cp.hist = ptr<void>(hist, "hist"); cp.words = ptr<int>(words, "words"); cp.cap = (int)cap; cp.N = (int)N;
}

// ... of a mixing op (rank_cache_frames, predict_cache_rows), with their bounds -- `steps` positions behind `pos`, which the message
// calls `pos_text` -- and theta, lam, ld_s
template <class Plan>
void mix_ring_into(const char *op, Plan &cp, int64_t H, int64_t R, const Tensor &hist, const Tensor &words, int64_t cap, int64_t pos,
                   int64_t steps, const char *pos_text, int64_t N, double theta, double lam, int64_t ld_s) {
    TORCH_CHECK(N >= 1 && N <= JLM_CACHE_MIX_MAX_N && cap >= N && cap <= INT32_MAX && pos >= 0 && pos + steps + cap < INT32_MAX && ld_s >= N &&
                    ld_s <= INT32_MAX,
                "jlm.", op, ": 1 <= N <= ", JLM_CACHE_MIX_MAX_N, ", cap >= N, ld_s >= N, ", pos_text, " + cap < 2^31");
    TORCH_CHECK(theta >= 0.0 && theta < 3.0e38 && lam >= 0.0 && lam < 1.0, "jlm.", op, ": theta finite and >= 0, lam in [0, 1)");
    ring_into(op, cp, H, R, hist, words, cap, N);
    cp.theta = (float)theta; cp.lam = (float)lam; cp.ld_s = (int)ld_s;
}

// score_frames with the continuous cache (jlm_score_cache_frames, include/jlm_hip.h): its arguments, then the rings hist
// [cap][n_rows][H] (4-byte values, the model's state-row format) and words [cap][n_rows] int32 with the carried entries in their slots,
// pos0, first / len [n_rows] int32 on the device, N, thetas (host), lpc [n_theta][n_steps][n_rows] float32, cache_flags one int32.
// -> as score_frames (the timed brackets are the scoring steps'; the cache pass runs behind the last).
Tensor score_cache_frames(const c10::intrusive_ptr<JlmModel> &model, const Tensor &h0, const Tensor &c0, const Tensor &h1, const Tensor &c1,
                          const OptTensor &T, const OptTensor &Tm, int64_t ld_tm, const OptTensor &part, int64_t max_parts, const Tensor &rows,
                          const Tensor &prev0, const Tensor &word, const Tensor &target, const Tensor &n_live, std::vector<int64_t> n_live_host,
                          const Tensor &nll_seq, const OptTensor &nll_tok, const OptTensor &flags, int64_t n_rows, int64_t n_steps, bool timed,
                          const Tensor &hist, const Tensor &words, int64_t cap, int64_t pos0, const Tensor &first, const Tensor &len, int64_t N,
                          std::vector<double> thetas, const Tensor &lpc, const OptTensor &cache_flags) {
    const jlm_decode_model &m = model->m;
    const int64_t R = n_rows, S = n_steps;
    const ScorePlanArgs sp("score_cache_frames", m, h0, c0, h1, c1, T, Tm, ld_tm, part, max_parts, rows, prev0, word, target, n_live,
                           n_live_host, nll_seq, nll_tok, flags, R, S);
    const int64_t n_theta = (int64_t)thetas.size();
    TORCH_CHECK(n_theta >= 1 && n_theta <= JLM_CACHE_MAX_THETAS, "jlm.score_cache_frames: 1 .. ", JLM_CACHE_MAX_THETAS, " values of theta");
    TORCH_CHECK(N >= 1 && cap >= N + S && cap <= INT32_MAX && pos0 >= 0 && pos0 + S + cap < INT32_MAX,
                "jlm.score_cache_frames: N >= 1, cap >= N + n_steps, 0 <= pos0, pos0 + n_steps + cap < 2^31");
    jlm_cache_plan cp{};
    ring_into("score_cache_frames", cp, m.H, R, hist, words, cap, N);
    TORCH_CHECK(is(first, at::kInt, R) && is(len, at::kInt, R) && is(lpc, at::kFloat, n_theta * S * R) && opt_ok(cache_flags, at::kInt, 1),
                "jlm.score_cache_frames: int32 first / len [n_rows], float32 lpc [n_theta][n_steps][n_rows], int32 cache_flags");
    std::vector<float> th(thetas.begin(), thetas.end());
    cp.pos0 = (int)pos0; cp.first = ptr<const int>(first, "first"); cp.len = ptr<const int>(len, "len");
    cp.thetas = th.data(); cp.n_theta = (int)n_theta;
    cp.lpc = ptr<float>(lpc, "lpc"); cp.flags = optr<int>(cache_flags, "cache_flags");
    return launch_frames("jlm_score_cache_frames", h0.device().index(), timed, R > 0 ? S : 0, JLM_SCORE_EVENTS_PER_STEP,
                         [&](hipStream_t st, void *const *ev) { return jlm_score_cache_frames(&m, &sp.p, &cp, st, ev); });
}

// score_frames against a memory of hidden states (jlm_score_memory_frames, include/jlm_hip.h): its arguments, then the memory keys
// [N][H] (4-byte values, the model's state-row format) and key_words [N] int32, the query rows q_rows [n_steps][n_rows][H] / q_words
// [n_steps][n_rows] the loop writes, len [n_rows] int32 on the device, thetas (host), lpm [n_theta][n_steps][n_rows] float32, the
// workspace (float32, jlm_memory_workspace_bytes) and mem_flags, one int32.  -> as score_frames (the memory pass runs behind the last
// step's bracket).
Tensor score_memory_frames(const c10::intrusive_ptr<JlmModel> &model, const Tensor &h0, const Tensor &c0, const Tensor &h1, const Tensor &c1,
                           const OptTensor &T, const OptTensor &Tm, int64_t ld_tm, const OptTensor &part, int64_t max_parts, const Tensor &rows,
                           const Tensor &prev0, const Tensor &word, const Tensor &target, const Tensor &n_live, std::vector<int64_t> n_live_host,
                           const Tensor &nll_seq, const OptTensor &nll_tok, const OptTensor &flags, int64_t n_rows, int64_t n_steps, bool timed,
                           const Tensor &keys, const Tensor &key_words, int64_t N, const Tensor &q_rows, const Tensor &q_words, const Tensor &len,
                           std::vector<double> thetas, const Tensor &lpm, const Tensor &workspace, const OptTensor &mem_flags) {
    const jlm_decode_model &m = model->m;
    const int64_t R = n_rows, S = n_steps;
    const ScorePlanArgs sp("score_memory_frames", m, h0, c0, h1, c1, T, Tm, ld_tm, part, max_parts, rows, prev0, word, target, n_live,
                           n_live_host, nll_seq, nll_tok, flags, R, S);
    const int64_t n_theta = (int64_t)thetas.size();
    TORCH_CHECK(n_theta >= 1 && n_theta <= JLM_CACHE_MAX_THETAS, "jlm.score_memory_frames: 1 .. ", JLM_CACHE_MAX_THETAS, " values of theta");
    TORCH_CHECK(N >= 1 && N <= JLM_MEMORY_MAX_KEYS, "jlm.score_memory_frames: 1 <= N <= ", JLM_MEMORY_MAX_KEYS);
    TORCH_CHECK(keys.defined() && keys.element_size() == 4 && keys.numel() >= N * (int64_t)m.H && is(key_words, at::kInt, N),
                "jlm.score_memory_frames: keys [N][H] of 4-byte values, int32 key_words [N]");
    TORCH_CHECK(q_rows.defined() && q_rows.element_size() == 4 && q_rows.numel() >= S * R * (int64_t)m.H && is(q_words, at::kInt, S * R),
                "jlm.score_memory_frames: q_rows [n_steps][n_rows][H] of 4-byte values, int32 q_words [n_steps][n_rows]");
    const size_t need = jlm_memory_workspace_bytes((int)N, (int)R, (int)S, (int)n_theta);
    TORCH_CHECK(is(len, at::kInt, R) && is(lpm, at::kFloat, n_theta * S * R) && opt_ok(mem_flags, at::kInt, 1) &&
                    is(workspace, at::kFloat, (int64_t)(need / 4)),
                "jlm.score_memory_frames: int32 len [n_rows], float32 lpm [n_theta][n_steps][n_rows], a float32 workspace of "
                "jlm_memory_workspace_bytes, int32 mem_flags");
    std::vector<float> th(thetas.begin(), thetas.end());
    jlm_memory_plan mp{};
    mp.keys = ptr<const void>(keys, "keys"); mp.key_words = ptr<const int>(key_words, "key_words"); mp.N = (int)N;
    mp.q_rows = ptr<void>(q_rows, "q_rows"); mp.q_words = ptr<int>(q_words, "q_words"); mp.len = ptr<const int>(len, "len");
    mp.thetas = th.data(); mp.n_theta = (int)n_theta;
    mp.lpm = ptr<float>(lpm, "lpm"); mp.workspace = ptr<void>(workspace, "workspace"); mp.workspace_bytes = (size_t)workspace.numel() * 4;
    mp.flags = optr<int>(mem_flags, "mem_flags");
    return launch_frames("jlm_score_memory_frames", h0.device().index(), timed, R > 0 ? S : 0, JLM_SCORE_EVENTS_PER_STEP,
                         [&](hipStream_t st, void *const *ev) { return jlm_score_memory_frames(&m, &sp.p, &mp, st, ev); });
}

// The level table of jlm_rank_rows as tensors, checked: ids [n_ids], lv_off [n_cols + 1], lv_lo / lv_hi of one length, all int32 on the
// device; without lv_off the other three are not passed on.
struct RankLevels {
    const int *ids = nullptr, *off = nullptr, *lo = nullptr, *hi = nullptr;
    int n_ids = 0;
    RankLevels(const char *op, const OptTensor &ids_t, const OptTensor &lv_off, const OptTensor &lv_lo, const OptTensor &lv_hi, int64_t n_cols,
               int64_t n_levels) {
        auto is_int = [&](const OptTensor &t, int64_t n) { return has(t) && t->scalar_type() == at::kInt && t->numel() >= n; };
        TORCH_CHECK(n_levels >= 0 && n_levels <= JLM_RANK_MAX_LEVELS, "jlm.", op, ": n_levels in 0 .. ", JLM_RANK_MAX_LEVELS);
        if (!has(lv_off)) return;
        TORCH_CHECK(is_int(lv_off, n_cols + 1) && is_int(lv_lo, 0) && is_int(lv_hi, 0) && lv_lo->numel() == lv_hi->numel() && is_int(ids_t, 0) &&
                        ids_t->numel() <= INT32_MAX,
                    "jlm.", op, ": int32 ids [n_ids], lv_off [n_cols + 1], lv_lo / lv_hi of one length");
        off = ptr<const int>(*lv_off, "lv_off");
        n_ids = (int)ids_t->numel();
        // (an empty table still hands the entry point pointers: it reads none of them through an empty span)
        ids = n_ids ? ptr<const int>(*ids_t, "ids") : nullptr;
        lo = lv_lo->numel() ? ptr<const int>(*lv_lo, "lv_lo") : off;
        hi = lv_hi->numel() ? ptr<const int>(*lv_hi, "lv_hi") : off;
    }
};

// the rank of target[r] in row r of f32 logits y [n_rows, ld] at every level of its level list (jlm_rank_rows, include/jlm_hip.h):
// rank int32 [n_rows, n_levels + 1].
void rank_rows(const Tensor &y, int64_t ld, int64_t n_cols, int64_t n_rows, const OptTensor &n_dev, const Tensor &target,
               const OptTensor &ids, const OptTensor &lv_off, const OptTensor &lv_lo, const OptTensor &lv_hi, int64_t n_levels,
               const Tensor &rank, const OptTensor &flags) {
    TORCH_CHECK(n_rows >= 0 && n_cols >= 1 && ld >= 0 && is(y, at::kFloat, n_rows * ld), "jlm.rank_rows: y [n_rows, ld] float32");
    const RankLevels lv("rank_rows", ids, lv_off, lv_lo, lv_hi, n_cols, n_levels);
    TORCH_CHECK(is(target, at::kInt, n_rows) && is(rank, at::kInt, n_rows * (n_levels + 1)) && opt_ok(n_dev, at::kInt, 1) &&
                    opt_ok(flags, at::kInt, 1),
                "jlm.rank_rows: int32 target [n_rows], rank [n_rows, n_levels + 1], n_dev / flags [1]");
    const c10::hip::HIPGuard device_guard(y.device().index());
    jlm_check(jlm_rank_rows(ptr<const float>(y, "y"), (int)ld, (int)n_cols, (int)n_rows, optr<const int>(n_dev, "n_dev"),
                            ptr<const int>(target, "target"), lv.ids, lv.n_ids, lv.off, lv.lo, lv.hi, (int)n_levels, ptr<int>(rank, "rank"),
                            optr<int>(flags, "flags"), stream_of(y)),
              "jlm_rank_rows");
}

// teacher-forced ranking of n_rows sequences / streams over n_steps steps (jlm_rank_frames, include/jlm_hip.h): score_frames' state row
// sets, rows / prev0 / word / target / n_live, generate_frames' logits [n_rows, ld_logits], rank_rows' level table; rank int32
// [n_steps][n_rows][n_levels + 1].  Every id must lie in [0, V): the caller checks (jlm_amd/rank.py).  -> timed: [n_steps, 4]
// milliseconds per step (LSTM step, T projection, logit GEMMs, ranking) after waiting for the last step; else an empty tensor.
// (the checked jlm_rank_plan of rank_frames and rank_cache_frames)
struct RankPlanArgs : ForcedPlanArgs<jlm_rank_plan> {
    int64_t V = 0;
    RankPlanArgs(const char *op, const jlm_decode_model &m, const Tensor &h0, const Tensor &c0, const Tensor &h1, const Tensor &c1,
                 const OptTensor &T, const Tensor &logits, int64_t ld_logits, const Tensor &rows, const Tensor &prev0, const Tensor &word,
                 const Tensor &target, const Tensor &n_live, const std::vector<int64_t> &n_live_host, const OptTensor &ids,
                 const OptTensor &lv_off, const OptTensor &lv_lo, const OptTensor &lv_hi, int64_t n_levels, const Tensor &rank,
                 const OptTensor &flags, int64_t R, int64_t S)
        : ForcedPlanArgs(op, m, h0, c0, h1, c1, T, rows, prev0, word, target, n_live, n_live_host, R, S) {
        TORCH_CHECK(m.n_segs >= 1, "jlm.", op, ": a model without segments");
        V = m.segs[m.n_segs - 1].v_end;
        const RankLevels lv(op, ids, lv_off, lv_lo, lv_hi, V, n_levels);
        TORCH_CHECK(is(rank, at::kInt, S * R * (n_levels + 1)) && opt_ok(flags, at::kInt, 1),
                    "jlm.", op, ": int32 rank [n_steps][n_rows][n_levels + 1], int32 flags");
        TORCH_CHECK(ld_logits >= 0 && is(logits, at::kFloat, R * ld_logits), "jlm.", op, ": logits [n_rows, ld_logits] float32");
        p.logits = ptr<float>(logits, "logits"); p.ld_logits = (int)ld_logits;
        p.ids = lv.ids; p.n_ids = lv.n_ids; p.lv_off = lv.off; p.lv_lo = lv.lo; p.lv_hi = lv.hi; p.n_levels = (int)n_levels;
        p.rank = ptr<int>(rank, "rank"); p.flags = optr<int>(flags, "flags");
    }
};

Tensor rank_frames(const c10::intrusive_ptr<JlmModel> &model, const Tensor &h0, const Tensor &c0, const Tensor &h1, const Tensor &c1,
                   const OptTensor &T, const Tensor &logits, int64_t ld_logits, const Tensor &rows, const Tensor &prev0, const Tensor &word,
                   const Tensor &target, const Tensor &n_live, std::vector<int64_t> n_live_host, const OptTensor &ids, const OptTensor &lv_off,
                   const OptTensor &lv_lo, const OptTensor &lv_hi, int64_t n_levels, const Tensor &rank, const OptTensor &flags, int64_t n_rows,
                   int64_t n_steps, bool timed) {
    const jlm_decode_model &m = model->m;
    const int64_t R = n_rows, S = n_steps;
    const RankPlanArgs rp("rank_frames", m, h0, c0, h1, c1, T, logits, ld_logits, rows, prev0, word, target, n_live, n_live_host, ids, lv_off,
                          lv_lo, lv_hi, n_levels, rank, flags, R, S);
    return launch_frames("jlm_rank_frames", h0.device().index(), timed, R > 0 ? S : 0, JLM_RANK_EVENTS_PER_STEP,
                         [&](hipStream_t st, void *const *ev) { return jlm_rank_frames(&m, &rp.p, st, ev); });
}

// rank_frames under the continuous cache (jlm_rank_cache_frames, include/jlm_hip.h): its arguments, then the rings hist
// [cap][n_rows][H] (4-byte values, the model's state-row format) and words [cap][n_rows] int32 with the carried entries in their slots,
// pos0, first [n_rows] int32 on the device, N, theta, lam, the scratch s [n_rows][ld_s] float32, top_k with top_ids int32 / top_nll
// float64 [n_steps][n_rows][top_k] (top_k = 0: none), cache_flags one int32.  -> timed: [n_steps, 6] milliseconds per step (LSTM step,
// T projection, logit GEMMs, cache query, cache patch, ranking with the lists and the ring write); else an empty tensor.
Tensor rank_cache_frames(const c10::intrusive_ptr<JlmModel> &model, const Tensor &h0, const Tensor &c0, const Tensor &h1, const Tensor &c1,
                         const OptTensor &T, const Tensor &logits, int64_t ld_logits, const Tensor &rows, const Tensor &prev0,
                         const Tensor &word, const Tensor &target, const Tensor &n_live, std::vector<int64_t> n_live_host, const OptTensor &ids,
                         const OptTensor &lv_off, const OptTensor &lv_lo, const OptTensor &lv_hi, int64_t n_levels, const Tensor &rank,
                         const OptTensor &flags, int64_t n_rows, int64_t n_steps, bool timed, const Tensor &hist, const Tensor &words,
                         int64_t cap, int64_t pos0, const Tensor &first, int64_t N, double theta, double lam, const Tensor &s, int64_t ld_s,
                         int64_t top_k, const OptTensor &top_ids, const OptTensor &top_nll, const OptTensor &cache_flags) {
    const jlm_decode_model &m = model->m;
    const int64_t R = n_rows, S = n_steps;
    const RankPlanArgs rp("rank_cache_frames", m, h0, c0, h1, c1, T, logits, ld_logits, rows, prev0, word, target, n_live, n_live_host, ids,
                          lv_off, lv_lo, lv_hi, n_levels, rank, flags, R, S);
    jlm_cache_mix_plan cp{};
    mix_ring_into("rank_cache_frames", cp, m.H, R, hist, words, cap, pos0, S, "0 <= pos0, pos0 + n_steps", N, theta, lam, ld_s);
    TORCH_CHECK(is(first, at::kInt, R) && is(s, at::kFloat, R * ld_s) && opt_ok(cache_flags, at::kInt, 1),
                "jlm.rank_cache_frames: int32 first [n_rows], float32 s [n_rows][ld_s], int32 cache_flags");
    TORCH_CHECK(top_k >= 0 && top_k <= JLM_TOPK_MAX && top_k <= rp.V &&
                    (top_k == 0 || (has(top_ids) && has(top_nll) && is(*top_ids, at::kInt, S * R * top_k) && is(*top_nll, at::kDouble, S * R * top_k))),
                "jlm.rank_cache_frames: top_k in 0 .. min(", JLM_TOPK_MAX, ", V) with int32 top_ids / float64 top_nll [n_steps][n_rows][top_k]");
    cp.pos0 = (int)pos0; cp.first = ptr<const int>(first, "first"); cp.s = ptr<float>(s, "s"); cp.top_k = (int)top_k;
    cp.top_ids = top_k > 0 ? ptr<int>(*top_ids, "top_ids") : nullptr; cp.top_nll = top_k > 0 ? ptr<double>(*top_nll, "top_nll") : nullptr;
    cp.flags = optr<int>(cache_flags, "cache_flags");
    return launch_frames("jlm_rank_cache_frames", h0.device().index(), timed, R > 0 ? S : 0, JLM_RANK_CACHE_EVENTS_PER_STEP,
                         [&](hipStream_t st, void *const *ev) { return jlm_rank_cache_frames(&m, &rp.p, &cp, st, ev); });
}

// The memory and the retrieval's buffers of a mixing op (rank_memory_frames, predict_memory_rows), checked, into its plan
// (jlm_memory_mix_plan, jlm_predict_memory_plan): `n_idx` sets of ret_idx [K][n_rows].
template <class Plan>
void memory_mix_into(const char *op, Plan &mp, int64_t H, int64_t R, const Tensor &keys, const Tensor &key_words, int64_t N, double theta,
                     double lam, int64_t K, const Tensor &s, int64_t ld_s, const Tensor &ret_words, const OptTensor &ret_idx, int64_t n_idx,
                     const Tensor &first, const Tensor &workspace, const OptTensor &mem_flags) {
    TORCH_CHECK(N >= 1 && N <= JLM_MEMORY_MAX_KEYS && K >= 1 && K <= JLM_MEMORY_TOPK_MAX && ld_s >= K && ld_s <= INT32_MAX && R <= 65535,
                "jlm.", op, ": 1 <= N <= ", JLM_MEMORY_MAX_KEYS, ", 1 <= K <= ", JLM_MEMORY_TOPK_MAX, ", ld_s >= K, n_rows <= 65535");
    TORCH_CHECK(theta >= 0.0 && theta < 3.0e38 && lam >= 0.0 && lam < 1.0, "jlm.", op, ": theta finite and >= 0, lam in [0, 1)");
    TORCH_CHECK(keys.defined() && keys.element_size() == 4 && keys.numel() >= N * H && is(key_words, at::kInt, N),
                "jlm.", op, ": keys [N][H] of 4-byte values, int32 key_words [N]");
    const size_t need = jlm_memory_topk_workspace_bytes((int)N, (int)R, (int)K);
    TORCH_CHECK(is(s, at::kFloat, R * ld_s) && is(ret_words, at::kInt, K * R) && opt_ok(ret_idx, at::kInt, n_idx * K * R) && is(first, at::kInt, R) &&
                    is(workspace, at::kFloat, (int64_t)(need / 4)) && opt_ok(mem_flags, at::kInt, 1),
                "jlm.", op, ": float32 s [n_rows][ld_s], int32 ret_words / ret_idx [K][n_rows], int32 first [n_rows], a float32 workspace of "
                "jlm_memory_topk_workspace_bytes, int32 mem_flags");
    mp.keys = ptr<const void>(keys, "keys"); mp.key_words = ptr<const int>(key_words, "key_words"); mp.N = (int)N;
    mp.theta = (float)theta; mp.lam = (float)lam; mp.K = (int)K;
    mp.s = ptr<float>(s, "s"); mp.ld_s = (int)ld_s; mp.ret_words = ptr<int>(ret_words, "ret_words"); mp.ret_idx = optr<int>(ret_idx, "ret_idx");
    mp.first = ptr<const int>(first, "first"); mp.workspace = ptr<void>(workspace, "workspace");
    mp.workspace_bytes = (size_t)workspace.numel() * 4;
}

// rank_frames under a memory (jlm_rank_memory_frames, include/jlm_hip.h): its arguments, then the memory keys [N][H] / key_words [N],
// theta, lam, K, the scratch s [n_rows][ld_s] float32 and ret_words [K][n_rows] int32, ret_idx int32 [K][n_rows] (keep_idx:
// [n_steps][K][n_rows], every step's neighbours), first [n_rows] int32 zeros, the workspace, top_k with top_ids int32 / top_nll float64
// [n_steps][n_rows][top_k] (top_k = 0: none), mem_flags one int32.  -> timed: [n_steps, 6] milliseconds per step (LSTM step, T
// projection, logit GEMMs, retrieval, patch, ranking with the lists); else an empty tensor.
Tensor rank_memory_frames(const c10::intrusive_ptr<JlmModel> &model, const Tensor &h0, const Tensor &c0, const Tensor &h1, const Tensor &c1,
                          const OptTensor &T, const Tensor &logits, int64_t ld_logits, const Tensor &rows, const Tensor &prev0,
                          const Tensor &word, const Tensor &target, const Tensor &n_live, std::vector<int64_t> n_live_host, const OptTensor &ids,
                          const OptTensor &lv_off, const OptTensor &lv_lo, const OptTensor &lv_hi, int64_t n_levels, const Tensor &rank,
                          const OptTensor &flags, int64_t n_rows, int64_t n_steps, bool timed, const Tensor &keys, const Tensor &key_words,
                          int64_t N, double theta, double lam, int64_t K, const Tensor &s, int64_t ld_s, const Tensor &ret_words,
                          const Tensor &ret_idx, bool keep_idx, const Tensor &first, const Tensor &workspace, int64_t top_k,
                          const OptTensor &top_ids, const OptTensor &top_nll, const OptTensor &mem_flags) {
    const jlm_decode_model &m = model->m;
    const int64_t R = n_rows, S = n_steps;
    const RankPlanArgs rp("rank_memory_frames", m, h0, c0, h1, c1, T, logits, ld_logits, rows, prev0, word, target, n_live, n_live_host, ids,
                          lv_off, lv_lo, lv_hi, n_levels, rank, flags, R, S);
    jlm_memory_mix_plan mp{};
    memory_mix_into("rank_memory_frames", mp, m.H, R, keys, key_words, N, theta, lam, K, s, ld_s, ret_words, ret_idx, keep_idx ? S : 1, first,
                    workspace, mem_flags);
    TORCH_CHECK(top_k >= 0 && top_k <= JLM_TOPK_MAX && top_k <= rp.V &&
                    (top_k == 0 || (has(top_ids) && has(top_nll) && is(*top_ids, at::kInt, S * R * top_k) && is(*top_nll, at::kDouble, S * R * top_k))),
                "jlm.rank_memory_frames: top_k in 0 .. min(", JLM_TOPK_MAX, ", V) with int32 top_ids / float64 top_nll [n_steps][n_rows][top_k]");
    mp.keep_idx = keep_idx ? 1 : 0; mp.top_k = (int)top_k;
    mp.top_ids = top_k > 0 ? ptr<int>(*top_ids, "top_ids") : nullptr; mp.top_nll = top_k > 0 ? ptr<double>(*top_nll, "top_nll") : nullptr;
    mp.flags = optr<int>(mem_flags, "mem_flags");
    return launch_frames("jlm_rank_memory_frames", h0.device().index(), timed, R > 0 ? S : 0, JLM_RANK_MEMORY_EVENTS_PER_STEP,
                         [&](hipStream_t st, void *const *ev) { return jlm_rank_memory_frames(&m, &rp.p, &mp, st, ev); });
}

// one draw per row of f32 logits y [n_rows, ld] (jlm_sample_rows, include/jlm_hip.h).  seed: the uint64 seed's bits as int64.
void sample_rows(const Tensor &y, int64_t ld, int64_t n_cols, int64_t n_rows, const OptTensor &n_dev, double temperature, int64_t seed,
                 int64_t step, const OptTensor &row_id, const OptTensor &forced, const OptTensor &done, int64_t stop_id, bool self_norm,
                 const Tensor &word, const Tensor &ids, const Tensor &nll, const OptTensor &flags) {
    TORCH_CHECK(n_rows >= 0 && n_cols >= 1 && is(y, at::kFloat, n_rows * ld), "jlm.sample_rows: y [n_rows, ld] float32");
    TORCH_CHECK(is(word, at::kInt, n_rows) && is(ids, at::kInt, n_rows) && is(nll, at::kDouble, n_rows) && opt_ok(n_dev, at::kInt, 1) &&
                    opt_ok(row_id, at::kInt, n_rows) && opt_ok(forced, at::kInt, n_rows) && opt_ok(done, at::kInt, n_rows) &&
                    opt_ok(flags, at::kInt, 1),
                "jlm.sample_rows: int32 word / ids / row_id / forced / done [n_rows], n_dev / flags [1]; float64 nll [n_rows]");
    const c10::hip::HIPGuard device_guard(y.device().index());
    jlm_check(jlm_sample_rows(ptr<const float>(y, "y"), (int)ld, (int)n_cols, (int)n_rows, optr<const int>(n_dev, "n_dev"), temperature,
                              (uint64_t)seed, (int)step, optr<const int>(row_id, "row_id"), optr<const int>(forced, "forced"),
                              optr<int>(done, "done"), (int)stop_id, self_norm ? 1 : 0, ptr<int>(word, "word"), ptr<int>(ids, "ids"),
                              ptr<double>(nll, "nll"), optr<int>(flags, "flags"), stream_of(y)),
              "jlm_sample_rows");
}

// sample_rows with a top-k / nucleus cut of the draw (jlm_sample_rows_trunc, include/jlm_hip.h): top_k <= 0 or >= n_cols and
// top_p >= 1 mean off.
void sample_rows_trunc(const Tensor &y, int64_t ld, int64_t n_cols, int64_t n_rows, const OptTensor &n_dev, double temperature,
                       int64_t seed, int64_t step, const OptTensor &row_id, const OptTensor &forced, const OptTensor &done,
                       int64_t stop_id, bool self_norm, int64_t top_k, double top_p, const Tensor &word, const Tensor &ids,
                       const Tensor &nll, const OptTensor &flags) {
    TORCH_CHECK(top_p > 0.0, "jlm.sample_rows_trunc: top_p in (0, 1] (>= 1: off)");
    TORCH_CHECK(n_rows >= 0 && n_cols >= 1 && is(y, at::kFloat, n_rows * ld), "jlm.sample_rows_trunc: y [n_rows, ld] float32");
    TORCH_CHECK(is(word, at::kInt, n_rows) && is(ids, at::kInt, n_rows) && is(nll, at::kDouble, n_rows) && opt_ok(n_dev, at::kInt, 1) &&
                    opt_ok(row_id, at::kInt, n_rows) && opt_ok(forced, at::kInt, n_rows) && opt_ok(done, at::kInt, n_rows) &&
                    opt_ok(flags, at::kInt, 1),
                "jlm.sample_rows_trunc: int32 word / ids / row_id / forced / done [n_rows], n_dev / flags [1]; float64 nll [n_rows]");
    const c10::hip::HIPGuard device_guard(y.device().index());
    const int k = (int)std::min<int64_t>(std::max<int64_t>(top_k, 0), INT32_MAX);
    jlm_check(jlm_sample_rows_trunc(ptr<const float>(y, "y"), (int)ld, (int)n_cols, (int)n_rows, optr<const int>(n_dev, "n_dev"),
                                    temperature, (uint64_t)seed, (int)step, optr<const int>(row_id, "row_id"),
                                    optr<const int>(forced, "forced"), optr<int>(done, "done"), (int)stop_id, self_norm ? 1 : 0, k, top_p,
                                    ptr<int>(word, "word"), ptr<int>(ids, "ids"), ptr<double>(nll, "nll"), optr<int>(flags, "flags"),
                                    stream_of(y)),
              "jlm_sample_rows_trunc");
}

// batched ancestral sampling (jlm_generate_frames, include/jlm_hip.h): state row sets h0/c0 and h1/c1 (ping-pong), T [n_rows, ldt]
// unless the model is untied f32, logits [n_rows, ld_logits]; rows / row_id / word / done [n_rows], prev / prompt [n_prompt][n_rows],
// n_live [n_prompt] int32 and its host copy; ids [n_words][n_rows] int32, nll [n_words][n_rows] f64, flags one int32.  Every id must
// lie in [0, V): the caller checks (jlm_amd/generate.py).  -> timed: [frames, 4] milliseconds per frame (LSTM step, T projection,
// logit GEMMs, draw) after waiting for the last frame; else an empty tensor and nothing waits.
// generate_frames_trunc: the same with every draw cut to its top_k words and then its top_p nucleus (jlm_generate_frames_trunc);
// top_k <= 0 (or >= V) and top_p >= 1 mean off, and with both off it is generate_frames.
Tensor generate_frames_trunc(const c10::intrusive_ptr<JlmModel> &model, const Tensor &h0, const Tensor &c0, const Tensor &h1,
                             const Tensor &c1, const OptTensor &T, const Tensor &logits, int64_t ld_logits, const Tensor &rows,
                             const Tensor &prev, const Tensor &prompt, const Tensor &n_live, std::vector<int64_t> n_live_host,
                             const Tensor &row_id, const Tensor &word, const OptTensor &done, int64_t stop_id, double temperature,
                             int64_t seed, const Tensor &ids, const Tensor &nll, const OptTensor &flags, int64_t n_rows, int64_t n_prompt,
                             int64_t n_words, bool timed, int64_t top_k, double top_p) {
    const jlm_decode_model &m = model->m;
    const int64_t R = n_rows, P = n_prompt, N = n_words;
    TORCH_CHECK(P >= 1 && N >= 0, "jlm.generate_frames: n_prompt >= 1 and n_words >= 0");
    TORCH_CHECK(top_p > 0.0, "jlm.generate_frames_trunc: top_p in (0, 1] (>= 1: off)");
    top_k = std::min<int64_t>(std::max<int64_t>(top_k, 0), INT32_MAX);
    check_row_sets("generate_frames", m, R, h0, c0, h1, c1, n_live_host, P, "prompt frame", R);
    TORCH_CHECK(is(rows, at::kInt, R) && is(row_id, at::kInt, R) && is(word, at::kInt, R) && (!has(done) || is(*done, at::kInt, R)) &&
                    is(prev, at::kInt, P * R) && is(prompt, at::kInt, P * R) && is(n_live, at::kInt, P),
                "jlm.generate_frames: int32 rows / row_id / word / done [n_rows], prev / prompt [n_prompt][n_rows], n_live [n_prompt]");
    TORCH_CHECK(is(ids, at::kInt, N * R) && is(nll, at::kDouble, N * R) && (!has(flags) || is(*flags, at::kInt, 1)),
                "jlm.generate_frames: int32 ids / float64 nll [n_words][n_rows], int32 flags");
    TORCH_CHECK(!has(T) || is(*T, at::kFloat, R * m.ldt), "jlm.generate_frames: T [n_rows, ldt] float32");
    TORCH_CHECK(is(logits, at::kFloat, R * ld_logits), "jlm.generate_frames: logits [n_rows, ld_logits] float32");
    jlm_generate_plan p{};
    p.n_rows = (int)R; p.n_prompt = (int)P; p.n_words = (int)N;
    p.h[0] = ptr<void>(h0, "h0"); p.h[1] = ptr<void>(h1, "h1"); p.c[0] = ptr<float>(c0, "c0"); p.c[1] = ptr<float>(c1, "c1");
    p.T = optr<float>(T, "T");
    p.logits = ptr<float>(logits, "logits"); p.ld_logits = (int)ld_logits;
    p.rows = ptr<const int>(rows, "rows"); p.prev = ptr<const int>(prev, "prev"); p.prompt = ptr<const int>(prompt, "prompt");
    p.n_live = ptr<const int>(n_live, "n_live");
    std::vector<int> live_host(n_live_host.begin(), n_live_host.end());
    p.n_live_host = live_host.data();
    p.row_id = ptr<const int>(row_id, "row_id"); p.word = ptr<int>(word, "word"); p.done = optr<int>(done, "done");
    p.stop_id = (int)stop_id; p.temperature = temperature; p.seed = (uint64_t)seed;
    p.ids = ptr<int>(ids, "ids"); p.nll = ptr<double>(nll, "nll"); p.flags = optr<int>(flags, "flags");
    const bool trunc = top_k > 0 || top_p < 1.0;
    return launch_frames(trunc ? "jlm_generate_frames_trunc" : "jlm_generate_frames", h0.device().index(), timed,
                         N > 0 && R > 0 ? P + N - 1 : 0, JLM_GENERATE_EVENTS_PER_FRAME, [&](hipStream_t st, void *const *ev) {
                             return trunc ? jlm_generate_frames_trunc(&m, &p, (int)top_k, top_p, st, ev) : jlm_generate_frames(&m, &p, st, ev);
                         });
}

Tensor generate_frames(const c10::intrusive_ptr<JlmModel> &model, const Tensor &h0, const Tensor &c0, const Tensor &h1, const Tensor &c1,
                       const OptTensor &T, const Tensor &logits, int64_t ld_logits, const Tensor &rows, const Tensor &prev,
                       const Tensor &prompt, const Tensor &n_live, std::vector<int64_t> n_live_host, const Tensor &row_id,
                       const Tensor &word, const OptTensor &done, int64_t stop_id, double temperature, int64_t seed, const Tensor &ids,
                       const Tensor &nll, const OptTensor &flags, int64_t n_rows, int64_t n_prompt, int64_t n_words, bool timed) {
    return generate_frames_trunc(model, h0, c0, h1, c1, T, logits, ld_logits, rows, prev, prompt, n_live, std::move(n_live_host), row_id,
                                 word, done, stop_id, temperature, seed, ids, nll, flags, n_rows, n_prompt, n_words, timed, 0, 1.0);
}

// the k best words of every row of f32 logits y [n_rows, ld] with their -log p (jlm_topk_rows, include/jlm_hip.h): ids int32 and nll
// float64 [n_rows, ld_out].
void topk_rows(const Tensor &y, int64_t ld, int64_t n_cols, int64_t n_rows, int64_t k, bool self_norm, const Tensor &ids, const Tensor &nll,
               int64_t ld_out, const OptTensor &flags) {
    TORCH_CHECK(n_rows >= 0 && n_cols >= 1 && is(y, at::kFloat, n_rows * ld), "jlm.topk_rows: y [n_rows, ld] float32");
    TORCH_CHECK(is(ids, at::kInt, n_rows * ld_out) && is(nll, at::kDouble, n_rows * ld_out) &&
                    (!flags.has_value() || !flags->defined() || is(*flags, at::kInt, 1)),
                "jlm.topk_rows: int32 ids / float64 nll [n_rows, ld_out], int32 flags [1]");
    const c10::hip::HIPGuard device_guard(y.device().index());
    jlm_check(jlm_topk_rows(ptr<const float>(y, "y"), (int)ld, (int)n_cols, (int)n_rows, (int)k, self_norm ? 1 : 0, ptr<int>(ids, "ids"),
                            ptr<double>(nll, "nll"), (int)ld_out, optr<int>(flags, "flags"), stream_of(y)),
              "jlm_topk_rows");
}

// the K nearest entries of a memory for every query row (jlm_memory_topk, include/jlm_hip.h): keys [N][H] of 4-byte values and int32
// key_words [N]; q_rows [n_rows][H] in the same format, every row live; s float32 [n_rows, ld_s], ret_words / ret_idx int32
// [K][n_rows]; the workspace float32 of at least jlm_memory_topk_workspace_bytes, flags one int32.
void memory_topk(const Tensor &keys, const Tensor &key_words, int64_t N, int64_t H, bool split, double h_scale, const Tensor &q_rows,
                 int64_t n_rows, double theta, int64_t K, const Tensor &s, int64_t ld_s, const Tensor &ret_words, const Tensor &ret_idx,
                 const Tensor &workspace, const OptTensor &flags) {
    TORCH_CHECK(N >= 1 && N <= JLM_MEMORY_MAX_KEYS && K >= 1 && K <= JLM_MEMORY_TOPK_MAX && ld_s >= K && ld_s <= INT32_MAX && H >= 1 &&
                    H <= INT32_MAX && n_rows >= 0 && n_rows <= 65535,
                "jlm.memory_topk: 1 <= N <= ", JLM_MEMORY_MAX_KEYS, ", 1 <= K <= ", JLM_MEMORY_TOPK_MAX, ", ld_s >= K, 0 <= n_rows <= 65535");
    TORCH_CHECK(theta >= 0.0 && theta < 3.0e38, "jlm.memory_topk: theta finite and >= 0");
    TORCH_CHECK(keys.defined() && keys.element_size() == 4 && keys.numel() >= N * H && is(key_words, at::kInt, N),
                "jlm.memory_topk: keys [N][H] of 4-byte values, int32 key_words [N]");
    TORCH_CHECK(q_rows.defined() && q_rows.element_size() == 4 && q_rows.numel() >= n_rows * H, "jlm.memory_topk: q_rows [n_rows][H] of 4-byte values");
    const size_t need = jlm_memory_topk_workspace_bytes((int)N, (int)n_rows, (int)K);
    TORCH_CHECK(is(s, at::kFloat, n_rows * ld_s) && is(ret_words, at::kInt, K * n_rows) && is(ret_idx, at::kInt, K * n_rows) &&
                    is(workspace, at::kFloat, (int64_t)(need / 4)) && opt_ok(flags, at::kInt, 1),
                "jlm.memory_topk: float32 s [n_rows, ld_s], int32 ret_words / ret_idx [K][n_rows], a float32 workspace of "
                "jlm_memory_topk_workspace_bytes, int32 flags");
    const c10::hip::HIPGuard device_guard(keys.device().index());
    jlm_check(jlm_memory_topk(ptr<const void>(keys, "keys"), ptr<const int>(key_words, "key_words"), (int)N, (int)H, split ? 1 : 0, (float)h_scale,
                              ptr<const void>(q_rows, "q_rows"), (int)n_rows, nullptr, (float)theta, (int)K, ptr<float>(s, "s"), (int)ld_s,
                              ptr<int>(ret_words, "ret_words"), ptr<int>(ret_idx, "ret_idx"), (int)n_rows, ptr<void>(workspace, "workspace"),
                              (size_t)workspace.numel() * 4, optr<int>(flags, "flags"), stream_of(keys)),
              "jlm_memory_topk");
}

// A word-set mask and its per-row set indices, checked on the host and the indices put on the device (jlm_topk_rows_masked, include/
// jlm_hip.h): mask int32 [n_sets, ld_mask] holding the 32-bit words' bits, row_set one index in [-1, n_sets) per row.
Tensor check_word_sets(const char *op, const Tensor &mask, int64_t ld_mask, int64_t n_sets, int64_t n_cols, const std::vector<int64_t> &row_set,
                       int64_t n_rows, const Tensor &like) {
    TORCH_CHECK(n_sets >= 0 && n_sets <= INT32_MAX && ld_mask >= 0 && ld_mask <= INT32_MAX && (n_sets == 0 || ld_mask >= (n_cols + 31) / 32) &&
                    mask.defined() && mask.scalar_type() == at::kInt && mask.numel() >= n_sets * ld_mask,
                "jlm.", op, ": mask int32 [n_sets, ld_mask] with ld_mask >= ceil(n_cols / 32) = ", (n_cols + 31) / 32);
    TORCH_CHECK((int64_t)row_set.size() == n_rows, "jlm.", op, ": one set index per row (", n_rows, ")");
    Tensor host = at::full({std::max<int64_t>(n_rows, 1)}, -1, at::kInt);      // (never empty: the entry point wants a pointer)
    for (size_t r = 0; r < row_set.size(); ++r) {
        TORCH_CHECK(row_set[r] >= -1 && row_set[r] < n_sets, "jlm.", op, ": set index ", row_set[r], " of row ", r, " outside [-1, ", n_sets, ")");
        host.data_ptr<int>()[r] = (int)row_set[r];
    }
    return host.to(like.device());
}

// topk_rows with row r restricted to the words of set row_set[r] of `mask` (jlm_topk_rows_masked, include/jlm_hip.h); -1: unrestricted.
void topk_rows_masked(const Tensor &y, int64_t ld, int64_t n_cols, int64_t n_rows, int64_t k, bool self_norm, const Tensor &mask,
                      int64_t ld_mask, int64_t n_sets, std::vector<int64_t> row_set, const Tensor &ids, const Tensor &nll, int64_t ld_out,
                      const OptTensor &flags) {
    TORCH_CHECK(n_rows >= 0 && n_cols >= 1 && is(y, at::kFloat, n_rows * ld), "jlm.topk_rows_masked: y [n_rows, ld] float32");
    TORCH_CHECK(is(ids, at::kInt, n_rows * ld_out) && is(nll, at::kDouble, n_rows * ld_out) &&
                    (!flags.has_value() || !flags->defined() || is(*flags, at::kInt, 1)),
                "jlm.topk_rows_masked: int32 ids / float64 nll [n_rows, ld_out], int32 flags [1]");
    const c10::hip::HIPGuard device_guard(y.device().index());
    on_gpu(y, "y");
    const Tensor sets = check_word_sets("topk_rows_masked", mask, ld_mask, n_sets, n_cols, row_set, n_rows, y);
    jlm_check(jlm_topk_rows_masked(ptr<const float>(y, "y"), (int)ld, (int)n_cols, (int)n_rows, (int)k, self_norm ? 1 : 0,
                                   n_sets > 0 ? ptr<const unsigned>(mask, "mask") : nullptr, (int)ld_mask, (int)n_sets,
                                   ptr<const int>(sets, "row_set"), ptr<int>(ids, "ids"), ptr<double>(nll, "nll"), (int)ld_out,
                                   optr<int>(flags, "flags"), stream_of(y)),
              "jlm_topk_rows_masked");
}

// One step of prediction under the continuous cache (jlm_predict_cache_rows, include/jlm_hip.h): h [n_rows, H] the carried state rows
// in the model's state-row format, the scratch T / logits / s, rows [n_rows] int32, the rings and their scalars as rank_cache_frames
// takes them with pos the streams' next position, k, and -- mask given -- the word sets of topk_rows_masked with one set index per
// row.  ids int32 / nll float64 [n_rows, k].  On the current stream; nothing waits.
void predict_cache_rows(const c10::intrusive_ptr<JlmModel> &model, const Tensor &h, const OptTensor &T, const Tensor &logits,
                        int64_t ld_logits, const Tensor &rows, const Tensor &hist, const Tensor &words, int64_t cap, int64_t pos,
                        const Tensor &first, int64_t N, double theta, double lam, const Tensor &s, int64_t ld_s, int64_t k,
                        const OptTensor &mask, int64_t ld_mask, int64_t n_sets, std::vector<int64_t> row_set, const Tensor &ids,
                        const Tensor &nll, const OptTensor &flags, const OptTensor &cache_flags, int64_t n_rows) {
    const jlm_decode_model &m = model->m;
    const int64_t R = n_rows;
    TORCH_CHECK(m.n_segs >= 1, "jlm.predict_cache_rows: a model without segments");
    TORCH_CHECK(!(m.untied && m.split_lstm), "jlm.predict_cache_rows: an untied split-row model keeps the f32 copy of its state, which its "
                                             "vocabulary GEMMs read, only inside the LSTM step: there is no one-step form for it");
    const int64_t V = m.segs[m.n_segs - 1].v_end;
    TORCH_CHECK(R >= 0 && R <= 65535 && h.defined() && h.element_size() == 4 && h.numel() >= R * m.H && is(rows, at::kInt, R),
                "jlm.predict_cache_rows: h [n_rows, H] of 4-byte values, int32 rows [n_rows], n_rows <= 65535");
    TORCH_CHECK(!has(T) || is(*T, at::kFloat, R * m.ldt), "jlm.predict_cache_rows: T [n_rows, ldt] float32");
    TORCH_CHECK(ld_logits >= 0 && is(logits, at::kFloat, R * ld_logits), "jlm.predict_cache_rows: logits [n_rows, ld_logits] float32");
    jlm_predict_cache_plan p{};
    mix_ring_into("predict_cache_rows", p, m.H, R, hist, words, cap, pos, 0, "0 <= pos, pos", N, theta, lam, ld_s);
    TORCH_CHECK(is(first, at::kInt, R) && is(s, at::kFloat, R * ld_s) && opt_ok(cache_flags, at::kInt, 1) && opt_ok(flags, at::kInt, 1),
                "jlm.predict_cache_rows: int32 first [n_rows], float32 s [n_rows][ld_s], int32 flags / cache_flags");
    TORCH_CHECK(k >= 1 && k <= JLM_TOPK_MAX && k <= V && is(ids, at::kInt, R * k) && is(nll, at::kDouble, R * k),
                "jlm.predict_cache_rows: k in 1 .. min(", JLM_TOPK_MAX, ", V), int32 ids / float64 nll [n_rows, k]");
    const c10::hip::HIPGuard device_guard(logits.device().index());
    on_gpu(logits, "logits");
    Tensor sets;
    if (has(mask)) sets = check_word_sets("predict_cache_rows", *mask, ld_mask, n_sets, V, row_set, R, logits);
    p.n_rows = (int)R; p.h = ptr<const void>(h, "h"); p.T = optr<float>(T, "T");
    p.logits = ptr<float>(logits, "logits"); p.ld_logits = (int)ld_logits; p.rows = ptr<const int>(rows, "rows");
    p.pos = (int)pos; p.first = ptr<const int>(first, "first"); p.s = ptr<float>(s, "s"); p.k = (int)k;
    if (has(mask)) {
        p.mask = n_sets > 0 ? ptr<const unsigned>(*mask, "mask") : nullptr; p.ld_mask = (int)ld_mask; p.n_sets = (int)n_sets;
        p.row_set = ptr<const int>(sets, "row_set");
    }
    p.ids = ptr<int>(ids, "ids"); p.nll = ptr<double>(nll, "nll"); p.flags = optr<int>(flags, "flags");
    p.cache_flags = optr<int>(cache_flags, "cache_flags");
    const std::lock_guard<std::mutex> lock(g_enqueue_mutex);
    jlm_check(jlm_predict_cache_rows(&m, &p, stream_of(logits)), "jlm_predict_cache_rows");
}

// One step of prediction under a memory (jlm_predict_memory_rows, include/jlm_hip.h): predict_cache_rows with the memory and the
// retrieval's buffers, as rank_memory_frames takes them, in the rings' place.  ids int32 / nll float64 [n_rows, k].
void predict_memory_rows(const c10::intrusive_ptr<JlmModel> &model, const Tensor &h, const OptTensor &T, const Tensor &logits,
                         int64_t ld_logits, const Tensor &rows, const Tensor &keys, const Tensor &key_words, int64_t N, double theta, double lam,
                         int64_t K, const Tensor &s, int64_t ld_s, const Tensor &ret_words, const OptTensor &ret_idx, const Tensor &first,
                         const Tensor &workspace, int64_t k, const OptTensor &mask, int64_t ld_mask, int64_t n_sets,
                         std::vector<int64_t> row_set, const Tensor &ids, const Tensor &nll, const OptTensor &flags, const OptTensor &mem_flags,
                         int64_t n_rows) {
    const jlm_decode_model &m = model->m;
    const int64_t R = n_rows;
    TORCH_CHECK(m.n_segs >= 1, "jlm.predict_memory_rows: a model without segments");
    TORCH_CHECK(!(m.untied && m.split_lstm), "jlm.predict_memory_rows: an untied split-row model keeps the f32 copy of its state, which its "
                                             "vocabulary GEMMs read, only inside the LSTM step: there is no one-step form for it");
    const int64_t V = m.segs[m.n_segs - 1].v_end;
    TORCH_CHECK(R >= 0 && R <= 65535 && h.defined() && h.element_size() == 4 && h.numel() >= R * m.H && is(rows, at::kInt, R),
                "jlm.predict_memory_rows: h [n_rows, H] of 4-byte values, int32 rows [n_rows], n_rows <= 65535");
    TORCH_CHECK(!has(T) || is(*T, at::kFloat, R * m.ldt), "jlm.predict_memory_rows: T [n_rows, ldt] float32");
    TORCH_CHECK(ld_logits >= 0 && is(logits, at::kFloat, R * ld_logits), "jlm.predict_memory_rows: logits [n_rows, ld_logits] float32");
    jlm_predict_memory_plan p{};
    memory_mix_into("predict_memory_rows", p, m.H, R, keys, key_words, N, theta, lam, K, s, ld_s, ret_words, ret_idx, 1, first, workspace,
                    mem_flags);
    TORCH_CHECK(opt_ok(flags, at::kInt, 1), "jlm.predict_memory_rows: int32 flags");
    TORCH_CHECK(k >= 1 && k <= JLM_TOPK_MAX && k <= V && is(ids, at::kInt, R * k) && is(nll, at::kDouble, R * k),
                "jlm.predict_memory_rows: k in 1 .. min(", JLM_TOPK_MAX, ", V), int32 ids / float64 nll [n_rows, k]");
    const c10::hip::HIPGuard device_guard(logits.device().index());
    on_gpu(logits, "logits");
    Tensor sets;
    if (has(mask)) sets = check_word_sets("predict_memory_rows", *mask, ld_mask, n_sets, V, row_set, R, logits);
    p.n_rows = (int)R; p.h = ptr<const void>(h, "h"); p.T = optr<float>(T, "T");
    p.logits = ptr<float>(logits, "logits"); p.ld_logits = (int)ld_logits; p.rows = ptr<const int>(rows, "rows"); p.k = (int)k;
    if (has(mask)) {
        p.mask = n_sets > 0 ? ptr<const unsigned>(*mask, "mask") : nullptr; p.ld_mask = (int)ld_mask; p.n_sets = (int)n_sets;
        p.row_set = ptr<const int>(sets, "row_set");
    }
    p.ids = ptr<int>(ids, "ids"); p.nll = ptr<double>(nll, "nll"); p.flags = optr<int>(flags, "flags");
    p.memory_flags = optr<int>(mem_flags, "mem_flags");
    const std::lock_guard<std::mutex> lock(g_enqueue_mutex);
    jlm_check(jlm_predict_memory_rows(&m, &p, stream_of(logits)), "jlm_predict_memory_rows");
}

// one beam selection per prompt over per-row top-`beam` lists (jlm_beam_merge, include/jlm_hip.h): cand_ids int32 / cand_nll float64
// [rows, beam]; word / prev / score (float64) / finished / bp_* [n_prompts * beam].
void beam_merge(const Tensor &cand_ids, const Tensor &cand_nll, int64_t beam, int64_t n_prompts, bool first, int64_t stop_id,
                const Tensor &word, const Tensor &prev, const Tensor &score, const Tensor &finished, const Tensor &bp_parent,
                const Tensor &bp_word, const Tensor &bp_nll) {
    const int64_t R = n_prompts * beam;
    TORCH_CHECK(beam >= 1 && n_prompts >= 0 && is(cand_ids, at::kInt, R * beam) && is(cand_nll, at::kDouble, R * beam),
                "jlm.beam_merge: cand_ids int32 / cand_nll float64 [n_prompts * beam, beam]");
    TORCH_CHECK(is(word, at::kInt, R) && is(prev, at::kInt, R) && is(score, at::kDouble, R) && is(finished, at::kInt, R) &&
                    is(bp_parent, at::kInt, R) && is(bp_word, at::kInt, R) && is(bp_nll, at::kDouble, R),
                "jlm.beam_merge: int32 word / prev / finished / bp_parent / bp_word, float64 score / bp_nll [n_prompts * beam]");
    const c10::hip::HIPGuard device_guard(cand_ids.device().index());
    jlm_check(jlm_beam_merge(ptr<const int>(cand_ids, "cand_ids"), ptr<const double>(cand_nll, "cand_nll"), (int)beam, (int)n_prompts,
                             first ? 1 : 0, (int)stop_id, ptr<int>(word, "word"), ptr<int>(prev, "prev"), ptr<double>(score, "score"),
                             ptr<int>(finished, "finished"), ptr<int>(bp_parent, "bp_parent"), ptr<int>(bp_word, "bp_word"),
                             ptr<double>(bp_nll, "bp_nll"), stream_of(cand_ids)),
              "jlm_beam_merge");
}

// beam-search completion (jlm_complete_frames, include/jlm_hip.h): state row sets h0/c0 and h1/c1 [R, H] (ping-pong, R = n_prompts *
// beam), T [R, ldt] unless the model is untied f32, logits [R, ld_logits]; rows [R], prev / prompt [n_prompt][n_prompts], n_live
// [n_prompt] int32 and its host copy; cand_ids / cand_nll [R, beam]; word / prev_row / score / finished [R]; bp_* [n_words][R]; flags
// one int32.  Every id must lie in [0, V): the caller checks (jlm_amd/complete.py).  -> timed: [frames, 5] milliseconds per frame (LSTM
// step, T projection, logit GEMMs, selection, merge) after waiting for the last frame; else an empty tensor and nothing waits.
// complete_frames_masked (jlm_complete_frames_masked): the same with prompt p's first word restricted to set prompt_set[p] of `mask`.
// (ngram: the n-gram plan of complete_frames_ngram, or NULL -- then the entry points are complete_frames' / complete_frames_masked's)
static Tensor complete_frames_any(const c10::intrusive_ptr<JlmModel> &model, const Tensor &h0, const Tensor &c0, const Tensor &h1, const Tensor &c1,
                       const OptTensor &T, const Tensor &logits, int64_t ld_logits, const Tensor &rows, const Tensor &prev,
                       const Tensor &prompt, const Tensor &n_live, std::vector<int64_t> n_live_host, const Tensor &cand_ids,
                       const Tensor &cand_nll, const Tensor &word, const Tensor &prev_row, const Tensor &score, const Tensor &finished,
                       int64_t stop_id, const Tensor &bp_parent, const Tensor &bp_word, const Tensor &bp_nll, const OptTensor &flags,
                       int64_t n_prompts, int64_t beam, int64_t n_prompt, int64_t n_words, bool timed, const OptTensor &mask,
                       int64_t ld_mask, int64_t n_sets, std::vector<int64_t> prompt_set, const jlm_complete_ngram_plan *ngram) {
    const jlm_decode_model &m = model->m;
    const int64_t NP = n_prompts, B = beam, P = n_prompt, N = n_words, R = n_prompts * beam;
    TORCH_CHECK(NP >= 0 && B >= 1 && P >= 1 && N >= 0, "jlm.complete_frames: n_prompts >= 0, beam >= 1, n_prompt >= 1 and n_words >= 0");
    check_row_sets("complete_frames", m, R, h0, c0, h1, c1, n_live_host, P, "prompt frame", NP);
    TORCH_CHECK(is(rows, at::kInt, R) && is(prev, at::kInt, P * NP) && is(prompt, at::kInt, P * NP) && is(n_live, at::kInt, P),
                "jlm.complete_frames: int32 rows [R], prev / prompt [n_prompt][n_prompts], n_live [n_prompt]");
    TORCH_CHECK(is(cand_ids, at::kInt, R * B) && is(cand_nll, at::kDouble, R * B) && is(word, at::kInt, R) && is(prev_row, at::kInt, R) &&
                    is(score, at::kDouble, R) && is(finished, at::kInt, R),
                "jlm.complete_frames: cand_ids int32 / cand_nll float64 [R, beam]; int32 word / prev_row / finished, float64 score [R]");
    TORCH_CHECK(is(bp_parent, at::kInt, N * R) && is(bp_word, at::kInt, N * R) && is(bp_nll, at::kDouble, N * R) &&
                    (!has(flags) || is(*flags, at::kInt, 1)),
                "jlm.complete_frames: int32 bp_parent / bp_word, float64 bp_nll [n_words][R], int32 flags");
    TORCH_CHECK(!has(T) || is(*T, at::kFloat, R * m.ldt), "jlm.complete_frames: T [R, ldt] float32");
    TORCH_CHECK(is(logits, at::kFloat, R * ld_logits), "jlm.complete_frames: logits [R, ld_logits] float32");
    jlm_complete_plan p{};
    p.n_prompts = (int)NP; p.beam = (int)B; p.n_prompt = (int)P; p.n_words = (int)N;
    p.h[0] = ptr<void>(h0, "h0"); p.h[1] = ptr<void>(h1, "h1"); p.c[0] = ptr<float>(c0, "c0"); p.c[1] = ptr<float>(c1, "c1");
    p.T = optr<float>(T, "T");
    p.logits = ptr<float>(logits, "logits"); p.ld_logits = (int)ld_logits;
    p.rows = ptr<const int>(rows, "rows"); p.prev = ptr<const int>(prev, "prev"); p.prompt = ptr<const int>(prompt, "prompt");
    p.n_live = ptr<const int>(n_live, "n_live");
    std::vector<int> live_host(n_live_host.begin(), n_live_host.end());
    p.n_live_host = live_host.data();
    p.cand_ids = ptr<int>(cand_ids, "cand_ids"); p.cand_nll = ptr<double>(cand_nll, "cand_nll");
    p.word = ptr<int>(word, "word"); p.prev_row = ptr<int>(prev_row, "prev_row");
    p.score = ptr<double>(score, "score"); p.finished = ptr<int>(finished, "finished");
    p.stop_id = (int)stop_id;
    p.bp_parent = ptr<int>(bp_parent, "bp_parent"); p.bp_word = ptr<int>(bp_word, "bp_word"); p.bp_nll = ptr<double>(bp_nll, "bp_nll");
    p.flags = optr<int>(flags, "flags");
    const bool masked = has(mask);
    Tensor sets;
    if (masked) {
        const c10::hip::HIPGuard device_guard(h0.device().index());
        on_gpu(logits, "logits");
        sets = check_word_sets("complete_frames_masked", *mask, ld_mask, n_sets, m.segs[m.n_segs - 1].v_end, prompt_set, NP, logits);
    }
    const unsigned *mask_p = masked && n_sets > 0 ? ptr<const unsigned>(*mask, "mask") : nullptr;
    const int *sets_p = masked ? ptr<const int>(sets, "prompt_set") : nullptr;
    if (ngram)
        return launch_frames("jlm_complete_frames_ngram", h0.device().index(), timed, N > 0 && NP > 0 ? P + N - 1 : 0,
                             JLM_COMPLETE_EVENTS_PER_FRAME, [&](hipStream_t st, void *const *ev) {
                                 return jlm_complete_frames_ngram(&m, &p, ngram, mask_p, masked ? (int)ld_mask : 0, masked ? (int)n_sets : 0,
                                                                  sets_p, st, ev);
                             });
    return launch_frames(masked ? "jlm_complete_frames_masked" : "jlm_complete_frames", h0.device().index(), timed,
                         N > 0 && NP > 0 ? P + N - 1 : 0, JLM_COMPLETE_EVENTS_PER_FRAME, [&](hipStream_t st, void *const *ev) {
                             return masked ? jlm_complete_frames_masked(&m, &p, mask_p, (int)ld_mask, (int)n_sets, sets_p, st, ev)
                                           : jlm_complete_frames(&m, &p, st, ev);
                         });
}

Tensor complete_frames_masked(const c10::intrusive_ptr<JlmModel> &model, const Tensor &h0, const Tensor &c0, const Tensor &h1, const Tensor &c1,
                       const OptTensor &T, const Tensor &logits, int64_t ld_logits, const Tensor &rows, const Tensor &prev,
                       const Tensor &prompt, const Tensor &n_live, std::vector<int64_t> n_live_host, const Tensor &cand_ids,
                       const Tensor &cand_nll, const Tensor &word, const Tensor &prev_row, const Tensor &score, const Tensor &finished,
                       int64_t stop_id, const Tensor &bp_parent, const Tensor &bp_word, const Tensor &bp_nll, const OptTensor &flags,
                       int64_t n_prompts, int64_t beam, int64_t n_prompt, int64_t n_words, bool timed, const OptTensor &mask,
                       int64_t ld_mask, int64_t n_sets, std::vector<int64_t> prompt_set) {
    return complete_frames_any(model, h0, c0, h1, c1, T, logits, ld_logits, rows, prev, prompt, n_live, std::move(n_live_host), cand_ids,
                               cand_nll, word, prev_row, score, finished, stop_id, bp_parent, bp_word, bp_nll, flags, n_prompts, beam,
                               n_prompt, n_words, timed, mask, ld_mask, n_sets, std::move(prompt_set), nullptr);
}

// The table of the n-gram row walk as tensors, checked, into a jlm_ngram_rows (include/jlm_hip.h; jlm_amd/ngram.py successor_tensors):
// table = [uni_lp, uni_bow, bi_off, bi_w, bi_lp, tri_off, tri_w, tri_lp, tri_bow, ctx_keys (int64), ctx_vals], sizes = [n_bi, n_tri,
// n_ctx, log2cap, max_probe]; an empty list is passed as a tensor of one element.
struct NgramRowsArgs {
    jlm_ngram_rows t{};
    NgramRowsArgs(const char *op, const std::vector<Tensor> &table, const std::vector<int64_t> &sizes, int64_t V, int64_t order, double lam,
                  const Tensor &like) {
        TORCH_CHECK(table.size() == 11 && sizes.size() == 5, "jlm.", op, ": the n-gram table is 11 tensors and 5 sizes");
        const int64_t n_bi = sizes[0], n_tri = sizes[1], n_ctx = sizes[2], log2cap = sizes[3], max_probe = sizes[4];
        TORCH_CHECK(order >= 1 && order <= 3 && lam > 0.0 && lam < 1.0, "jlm.", op, ": n-gram order in 1 .. 3 and lam in (0, 1)");
        TORCH_CHECK(V >= 1 && V <= JLM_NGRAM_MIX_MAX_V, "jlm.", op, ": the n-gram mixture over whole rows takes at most ", JLM_NGRAM_MIX_MAX_V,
                    " words");
        TORCH_CHECK(n_bi >= 0 && n_bi <= INT32_MAX && n_tri >= 0 && n_tri <= INT32_MAX && n_ctx >= 0 && n_ctx <= INT32_MAX && log2cap >= 6 &&
                        log2cap <= 31 && max_probe >= 0 && max_probe < (int64_t(1) << log2cap),
                    "jlm.", op, ": n-gram table sizes out of range");
        for (const Tensor &x : table) TORCH_CHECK(x.defined() && x.device() == like.device(), "jlm.", op, ": the n-gram table lives on the call's device");
        const int64_t one = 1, cap = int64_t(1) << log2cap;
        TORCH_CHECK(is(table[0], at::kFloat, V) && is(table[1], at::kFloat, V) && is(table[2], at::kInt, V + 1) &&
                        is(table[3], at::kInt, std::max(n_bi, one)) && is(table[4], at::kFloat, std::max(n_bi, one)) &&
                        is(table[5], at::kInt, n_ctx + 1) && is(table[6], at::kInt, std::max(n_tri, one)) &&
                        is(table[7], at::kFloat, std::max(n_tri, one)) && is(table[8], at::kFloat, std::max(n_ctx, one)) &&
                        is(table[9], at::kLong, cap) && is(table[10], at::kInt, cap),
                    "jlm.", op, ": float32 uni_lp / uni_bow [V], int32 bi_off [V + 1], bi_w / float32 bi_lp [n_bi], int32 tri_off [n_ctx + 1], "
                    "tri_w / float32 tri_lp [n_tri], tri_bow [n_ctx], int64 ctx_keys / int32 ctx_vals [2^log2cap]");
        t.uni_lp = ptr<const float>(table[0], "uni_lp"); t.uni_bow = ptr<const float>(table[1], "uni_bow");
        t.bi_off = ptr<const int>(table[2], "bi_off"); t.bi_w = ptr<const int>(table[3], "bi_w"); t.bi_lp = ptr<const float>(table[4], "bi_lp");
        t.n_bi = (int)n_bi;
        t.tri_off = ptr<const int>(table[5], "tri_off"); t.tri_w = ptr<const int>(table[6], "tri_w");
        t.tri_lp = ptr<const float>(table[7], "tri_lp"); t.tri_bow = ptr<const float>(table[8], "tri_bow");
        t.n_tri = (int)n_tri; t.n_ctx = (int)n_ctx;
        t.ctx_keys = ptr<const void>(table[9], "ctx_keys"); t.ctx_vals = ptr<const int>(table[10], "ctx_vals");
        t.log2cap = (int)log2cap; t.max_probe = (int)max_probe;
    }
};

// complete_frames / complete_frames_masked (mask None: the former) under the n-gram mixture (jlm_complete_frames_ngram, include/
// jlm_hip.h): their arguments, then the table (NgramRowsArgs), order, lam, hist0 / hist1 int32 [n_prompts * beam][2] -- hist0's first
// n_prompts rows the last two words of the prompts, -1 for no word --, ngram_flags one int32.
Tensor complete_frames_ngram(const c10::intrusive_ptr<JlmModel> &model, const Tensor &h0, const Tensor &c0, const Tensor &h1, const Tensor &c1,
                       const OptTensor &T, const Tensor &logits, int64_t ld_logits, const Tensor &rows, const Tensor &prev,
                       const Tensor &prompt, const Tensor &n_live, std::vector<int64_t> n_live_host, const Tensor &cand_ids,
                       const Tensor &cand_nll, const Tensor &word, const Tensor &prev_row, const Tensor &score, const Tensor &finished,
                       int64_t stop_id, const Tensor &bp_parent, const Tensor &bp_word, const Tensor &bp_nll, const OptTensor &flags,
                       int64_t n_prompts, int64_t beam, int64_t n_prompt, int64_t n_words, bool timed, const OptTensor &mask,
                       int64_t ld_mask, int64_t n_sets, std::vector<int64_t> prompt_set, std::vector<Tensor> table, std::vector<int64_t> sizes,
                       int64_t order, double lam, const Tensor &hist0, const Tensor &hist1, const OptTensor &ngram_flags) {
    const jlm_decode_model &m = model->m;
    TORCH_CHECK(m.n_segs >= 1, "jlm.complete_frames_ngram: a model without segments");
    const NgramRowsArgs tab("complete_frames_ngram", table, sizes, m.segs[m.n_segs - 1].v_end, order, lam, logits);
    const int64_t R = n_prompts * beam;
    TORCH_CHECK(n_prompts >= 0 && beam >= 1 && is(hist0, at::kInt, 2 * R) && is(hist1, at::kInt, 2 * R) && opt_ok(ngram_flags, at::kInt, 1) &&
                    (R == 0 || hist0.data_ptr() != hist1.data_ptr()),
                "jlm.complete_frames_ngram: two different int32 hist buffers [n_prompts * beam][2], int32 ngram_flags");
    jlm_complete_ngram_plan np{};
    np.table = &tab.t; np.order = (int)order; np.lam = (float)lam;
    np.hist[0] = ptr<int>(hist0, "hist0"); np.hist[1] = ptr<int>(hist1, "hist1"); np.flags = optr<int>(ngram_flags, "ngram_flags");
    return complete_frames_any(model, h0, c0, h1, c1, T, logits, ld_logits, rows, prev, prompt, n_live, std::move(n_live_host), cand_ids,
                               cand_nll, word, prev_row, score, finished, stop_id, bp_parent, bp_word, bp_nll, flags, n_prompts, beam,
                               n_prompt, n_words, timed, mask, ld_mask, n_sets, std::move(prompt_set), &np);
}

Tensor complete_frames(const c10::intrusive_ptr<JlmModel> &model, const Tensor &h0, const Tensor &c0, const Tensor &h1, const Tensor &c1,
                       const OptTensor &T, const Tensor &logits, int64_t ld_logits, const Tensor &rows, const Tensor &prev,
                       const Tensor &prompt, const Tensor &n_live, std::vector<int64_t> n_live_host, const Tensor &cand_ids,
                       const Tensor &cand_nll, const Tensor &word, const Tensor &prev_row, const Tensor &score, const Tensor &finished,
                       int64_t stop_id, const Tensor &bp_parent, const Tensor &bp_word, const Tensor &bp_nll, const OptTensor &flags,
                       int64_t n_prompts, int64_t beam, int64_t n_prompt, int64_t n_words, bool timed) {
    return complete_frames_masked(model, h0, c0, h1, c1, T, logits, ld_logits, rows, prev, prompt, n_live, std::move(n_live_host), cand_ids,
                                  cand_nll, word, prev_row, score, finished, stop_id, bp_parent, bp_word, bp_nll, flags, n_prompts, beam,
                                  n_prompt, n_words, timed, c10::nullopt, 0, 0, {});
}

// rank_frames under the n-gram mixture (jlm_rank_ngram_frames, include/jlm_hip.h): its arguments, then the table (NgramRowsArgs), order,
// lam, hist int32 [n_steps][n_rows][2] on the device, top_k with top_ids int32 / top_nll float64 [n_steps][n_rows][top_k] (top_k = 0:
// none), ngram_flags one int32.  -> timed: [n_steps, 5] milliseconds per step (LSTM step, T projection, logit GEMMs, n-gram patch,
// ranking with the lists); else an empty tensor.
Tensor rank_ngram_frames(const c10::intrusive_ptr<JlmModel> &model, const Tensor &h0, const Tensor &c0, const Tensor &h1, const Tensor &c1,
                         const OptTensor &T, const Tensor &logits, int64_t ld_logits, const Tensor &rows, const Tensor &prev0,
                         const Tensor &word, const Tensor &target, const Tensor &n_live, std::vector<int64_t> n_live_host, const OptTensor &ids,
                         const OptTensor &lv_off, const OptTensor &lv_lo, const OptTensor &lv_hi, int64_t n_levels, const Tensor &rank,
                         const OptTensor &flags, int64_t n_rows, int64_t n_steps, bool timed, std::vector<Tensor> table,
                         std::vector<int64_t> sizes, int64_t order, double lam, const Tensor &hist, int64_t top_k, const OptTensor &top_ids,
                         const OptTensor &top_nll, const OptTensor &ngram_flags) {
    const jlm_decode_model &m = model->m;
    const int64_t R = n_rows, S = n_steps;
    const RankPlanArgs rp("rank_ngram_frames", m, h0, c0, h1, c1, T, logits, ld_logits, rows, prev0, word, target, n_live, n_live_host, ids,
                          lv_off, lv_lo, lv_hi, n_levels, rank, flags, R, S);
    const NgramRowsArgs tab("rank_ngram_frames", table, sizes, rp.V, order, lam, logits);
    TORCH_CHECK(is(hist, at::kInt, S * R * 2) && opt_ok(ngram_flags, at::kInt, 1),
                "jlm.rank_ngram_frames: int32 hist [n_steps][n_rows][2], int32 ngram_flags");
    TORCH_CHECK(top_k >= 0 && top_k <= JLM_TOPK_MAX && top_k <= rp.V &&
                    (top_k == 0 || (has(top_ids) && has(top_nll) && is(*top_ids, at::kInt, S * R * top_k) && is(*top_nll, at::kDouble, S * R * top_k))),
                "jlm.rank_ngram_frames: top_k in 0 .. min(", JLM_TOPK_MAX, ", V) with int32 top_ids / float64 top_nll [n_steps][n_rows][top_k]");
    jlm_ngram_mix_plan np{};
    np.table = &tab.t; np.order = (int)order; np.lam = (float)lam; np.hist = ptr<const int>(hist, "hist"); np.top_k = (int)top_k;
    np.top_ids = top_k > 0 ? ptr<int>(*top_ids, "top_ids") : nullptr; np.top_nll = top_k > 0 ? ptr<double>(*top_nll, "top_nll") : nullptr;
    np.flags = optr<int>(ngram_flags, "ngram_flags");
    return launch_frames("jlm_rank_ngram_frames", h0.device().index(), timed, R > 0 ? S : 0, JLM_RANK_NGRAM_EVENTS_PER_STEP,
                         [&](hipStream_t st, void *const *ev) { return jlm_rank_ngram_frames(&m, &rp.p, &np, st, ev); });
}

// scalar k-means compression of one tensor (jlm_kmeans1d, include/jlm_hip.h): x float32 [n], code uint8 [n], codebook float32 [2^bit],
// scratch uint8 [JLM_KMEANS_SCRATCH_BYTES].  The op waits for its stream.  -> float64 [9] on the host: Lloyd passes, constant, non-finite,
// 0, then (timed) milliseconds of range, histogram, seeding, Lloyd passes, final assignment.
Tensor kmeans1d(const Tensor &x, int64_t bit, int64_t seed, int64_t max_iter, double tol, const Tensor &code, const Tensor &codebook,
                const Tensor &scratch, int64_t grid, bool timed) {
    const int64_t n = x.defined() ? x.numel() : 0;
    TORCH_CHECK(n >= 1 && n <= JLM_KMEANS_MAX_N && is(x, at::kFloat, n), "jlm.kmeans1d: x float32, 1 .. 2^27 values");
    TORCH_CHECK(bit >= 1 && bit <= 8 && max_iter >= 1 && max_iter <= INT32_MAX && seed >= 0 && grid >= 0 && grid <= (1 << 20),
                "jlm.kmeans1d: 1 <= bit <= 8, max_iter >= 1, seed >= 0, 0 <= grid <= 2^20");
    TORCH_CHECK(is(code, at::kByte, n) && is(codebook, at::kFloat, int64_t(1) << bit) && is(scratch, at::kByte, JLM_KMEANS_SCRATCH_BYTES),
                "jlm.kmeans1d: code uint8 [n], codebook float32 [2^bit], scratch uint8 [JLM_KMEANS_SCRATCH_BYTES]");
    const c10::hip::HIPGuard device_guard(x.device().index());
    int info[4] = {0, 0, 0, 0};
    float ms[5] = {0, 0, 0, 0, 0};
    jlm_check(jlm_kmeans1d(ptr<const float>(x, "x"), (long long)n, (int)bit, (uint64_t)seed, (int)max_iter, tol, ptr<unsigned char>(code, "code"),
                           ptr<float>(codebook, "codebook"), ptr<void>(scratch, "scratch"), (int)grid, info, timed ? ms : nullptr, stream_of(x)),
              "jlm_kmeans1d");
    Tensor out = at::zeros({9}, at::TensorOptions().dtype(at::kDouble));
    double *o = out.data_ptr<double>();
    for (int i = 0; i < 4; ++i) o[i] = info[i];
    for (int i = 0; i < 5; ++i) o[4 + i] = ms[i];
    return out;
}

// ---- training (csrc/jlm_train.hip; jlm_amd/train.py DeviceStepper).  The operands may be VIEWS of larger buffers (a row or column range of
// the flat parameter buffer, a chunk of the logits scratch): `reach` elements from the view's first must lie inside its storage.
template <class T> T *vptr(const Tensor &t, at::ScalarType ty, int64_t reach, const char *name) {
    TORCH_CHECK(t.defined() && t.is_cuda() && t.scalar_type() == ty, "jlm.train: `", name, "` must be a GPU tensor of the documented type");
    const int64_t have = (int64_t)(t.storage().nbytes() / t.element_size()) - t.storage_offset();
    TORCH_CHECK(reach >= 1 && reach <= have, "jlm.train: `", name, "` reaches ", reach, " elements, its storage holds ", have);
    return reinterpret_cast<T *>(t.data_ptr());
}
int64_t span(int64_t rows, int64_t ld, int64_t cols) { return (rows - 1) * ld + cols; }

void train_gemm(const Tensor &A, int64_t sam, int64_t sak, const Tensor &B, int64_t sbk, int64_t sbn, const Tensor &C, int64_t ldc, int64_t M,
                int64_t N, int64_t K, bool accumulate, const OptTensor &bias) {
    TORCH_CHECK(M >= 1 && N >= 1 && K >= 1 && M <= INT32_MAX && N <= INT32_MAX && K <= INT32_MAX && ldc >= N && ldc <= INT32_MAX && sam >= 1 &&
                sak >= 1 && sbk >= 1 && sbn >= 1, "jlm.train_gemm: bad shape");
    const c10::hip::HIPGuard device_guard(C.device().index());
    const bool has_bias = bias.has_value() && bias->defined();
    jlm_check(jlm_train_gemm(vptr<const float>(A, at::kFloat, (M - 1) * sam + (K - 1) * sak + 1, "A"), sam, sak,
                             vptr<const float>(B, at::kFloat, (K - 1) * sbk + (N - 1) * sbn + 1, "B"), sbk, sbn,
                             vptr<float>(C, at::kFloat, span(M, ldc, N), "C"), (int)ldc, (int)M, (int)N, (int)K, accumulate ? 1 : 0,
                             has_bias ? vptr<const float>(*bias, at::kFloat, N, "bias") : nullptr, stream_of(C)),
              "jlm_train_gemm");
}

void train_embed_rows(const Tensor &emb, int64_t ld_emb, int64_t V, const Tensor &ids, int64_t n_rows, int64_t E, const Tensor &x, int64_t key,
                      int64_t thr, double scale) {
    TORCH_CHECK(n_rows >= 1 && E >= 1 && ld_emb >= E && V >= 1 && V <= INT32_MAX && n_rows * E <= INT32_MAX && thr >= 0 && thr <= (1 << 24),
                "jlm.train_embed_rows: bad shape");
    const c10::hip::HIPGuard device_guard(x.device().index());
    jlm_check(jlm_train_embed_rows(vptr<const float>(emb, at::kFloat, span(V, ld_emb, E), "emb"), (int)ld_emb, (int)V,
                                   vptr<const int>(ids, at::kInt, n_rows, "ids"), (int)n_rows, (int)E, vptr<float>(x, at::kFloat, n_rows * E, "x"),
                                   (uint64_t)key, (unsigned)thr, (float)scale, stream_of(x)),
              "jlm_train_embed_rows");
}

void train_cell_fwd(const Tensor &z, const Tensor &c_prev, const Tensor &c, const Tensor &h, const Tensor &r, int64_t B, int64_t H, int64_t row0,
                    int64_t key, int64_t thr, double scale) {
    TORCH_CHECK(B >= 1 && H >= 1 && B * H * 4 <= INT32_MAX && row0 >= 0 && thr >= 0 && thr <= (1 << 24), "jlm.train_cell_fwd: bad shape");
    const c10::hip::HIPGuard device_guard(z.device().index());
    jlm_check(jlm_train_cell_fwd(vptr<float>(z, at::kFloat, 4 * B * H, "z"), vptr<const float>(c_prev, at::kFloat, B * H, "c_prev"),
                                 vptr<float>(c, at::kFloat, B * H, "c"), vptr<float>(h, at::kFloat, B * H, "h"), vptr<float>(r, at::kFloat, B * H, "r"),
                                 (int)B, (int)H, (long long)row0, (uint64_t)key, (unsigned)thr, (float)scale, stream_of(z)),
              "jlm_train_cell_fwd");
}

void train_cell_bwd(const Tensor &gates, const Tensor &c, const Tensor &c_prev, const Tensor &dr, const OptTensor &dh_next, const Tensor &dc,
                    const Tensor &dz, int64_t B, int64_t H, int64_t row0, int64_t key, int64_t thr, double scale) {
    TORCH_CHECK(B >= 1 && H >= 1 && B * H * 4 <= INT32_MAX && row0 >= 0 && thr >= 0 && thr <= (1 << 24), "jlm.train_cell_bwd: bad shape");
    const c10::hip::HIPGuard device_guard(dz.device().index());
    const bool has_next = dh_next.has_value() && dh_next->defined();
    jlm_check(jlm_train_cell_bwd(vptr<const float>(gates, at::kFloat, 4 * B * H, "gates"), vptr<const float>(c, at::kFloat, B * H, "c"),
                                 vptr<const float>(c_prev, at::kFloat, B * H, "c_prev"), vptr<const float>(dr, at::kFloat, B * H, "dr"),
                                 has_next ? vptr<const float>(*dh_next, at::kFloat, B * H, "dh_next") : nullptr,
                                 vptr<float>(dc, at::kFloat, B * H, "dc"), vptr<float>(dz, at::kFloat, 4 * B * H, "dz"), (int)B, (int)H,
                                 (long long)row0, (uint64_t)key, (unsigned)thr, (float)scale, stream_of(dz)),
              "jlm_train_cell_bwd");
}

void train_lse_update(const Tensor &y, int64_t ld, int64_t n_cols, int64_t n_rows, const Tensor &run_m, const Tensor &run_s, bool first) {
    TORCH_CHECK(n_cols >= 1 && n_rows >= 1 && ld >= n_cols && ld <= INT32_MAX && n_rows <= INT32_MAX, "jlm.train_lse_update: bad shape");
    const c10::hip::HIPGuard device_guard(y.device().index());
    jlm_check(jlm_train_lse_update(vptr<const float>(y, at::kFloat, span(n_rows, ld, n_cols), "y"), (int)ld, (int)n_cols, (int)n_rows,
                                   vptr<float>(run_m, at::kFloat, n_rows, "run_m"), vptr<float>(run_s, at::kFloat, n_rows, "run_s"),
                                   first ? 1 : 0, stream_of(y)),
              "jlm_train_lse_update");
}

void train_dy(const Tensor &y, int64_t ld, int64_t n_cols, int64_t v0, int64_t n_rows, const Tensor &run_m, const Tensor &run_s,
              const Tensor &target, const Tensor &tgt_logit, double s, double nw2) {
    TORCH_CHECK(n_cols >= 1 && n_rows >= 1 && n_rows <= 65535 && ld >= n_cols && ld <= INT32_MAX && v0 >= 0 && v0 + n_cols <= INT32_MAX,
                "jlm.train_dy: bad shape");
    const c10::hip::HIPGuard device_guard(y.device().index());
    jlm_check(jlm_train_dy(vptr<float>(y, at::kFloat, span(n_rows, ld, n_cols), "y"), (int)ld, (int)n_cols, (int)v0, (int)n_rows,
                           vptr<const float>(run_m, at::kFloat, n_rows, "run_m"), vptr<const float>(run_s, at::kFloat, n_rows, "run_s"),
                           vptr<const int>(target, at::kInt, n_rows, "target"), vptr<float>(tgt_logit, at::kFloat, n_rows, "tgt_logit"), (float)s,
                           (float)nw2, stream_of(y)),
              "jlm_train_dy");
}

void train_colsum(const Tensor &a, int64_t ld, int64_t n_rows, int64_t n_cols, const Tensor &out, bool accumulate) {
    TORCH_CHECK(n_cols >= 1 && n_rows >= 1 && ld >= n_cols && ld <= INT32_MAX && n_rows <= INT32_MAX, "jlm.train_colsum: bad shape");
    const c10::hip::HIPGuard device_guard(a.device().index());
    jlm_check(jlm_train_colsum(vptr<const float>(a, at::kFloat, span(n_rows, ld, n_cols), "a"), (int)ld, (int)n_rows, (int)n_cols,
                               vptr<float>(out, at::kFloat, n_cols, "out"), accumulate ? 1 : 0, stream_of(a)),
              "jlm_train_colsum");
}

void train_ce(const Tensor &run_m, const Tensor &run_s, const Tensor &tgt_logit, int64_t n_rows, double nw, const Tensor &ce_out,
              const Tensor &flag) {
    TORCH_CHECK(n_rows >= 1 && n_rows <= INT32_MAX, "jlm.train_ce: bad shape");
    const c10::hip::HIPGuard device_guard(run_m.device().index());
    jlm_check(jlm_train_ce(vptr<const float>(run_m, at::kFloat, n_rows, "run_m"), vptr<const float>(run_s, at::kFloat, n_rows, "run_s"),
                           vptr<const float>(tgt_logit, at::kFloat, n_rows, "tgt_logit"), (int)n_rows, (float)nw, vptr<double>(ce_out, at::kDouble, 1, "ce_out"),
                           vptr<int>(flag, at::kInt, 1, "flag"), stream_of(run_m)),
              "jlm_train_ce");
}

void train_distill_lse_update(const Tensor &ys, int64_t ld_s, const Tensor &yt, int64_t ld_t, int64_t n_cols, int64_t n_rows, double inv_tau,
                              const Tensor &run, bool first) {
    TORCH_CHECK(n_cols >= 1 && n_rows >= 1 && ld_s >= n_cols && ld_s <= INT32_MAX && ld_t >= n_cols && ld_t <= INT32_MAX && n_rows <= INT32_MAX &&
                inv_tau > 0.0 && std::isfinite(inv_tau), "jlm.train_distill_lse_update: bad shape");
    const c10::hip::HIPGuard device_guard(ys.device().index());
    jlm_check(jlm_distill_lse_update(vptr<const float>(ys, at::kFloat, span(n_rows, ld_s, n_cols), "ys"), (int)ld_s,
                                     vptr<const float>(yt, at::kFloat, span(n_rows, ld_t, n_cols), "yt"), (int)ld_t, (int)n_cols, (int)n_rows,
                                     (float)inv_tau, vptr<float>(run, at::kFloat, 6 * n_rows, "run"), first ? 1 : 0, stream_of(ys)),
              "jlm_distill_lse_update");
}

void train_distill_dy(const Tensor &ys, int64_t ld_s, const Tensor &yt, int64_t ld_t, int64_t n_cols, int64_t v0, int64_t n_rows, const Tensor &run,
                      const Tensor &target, const Tensor &tgt_logit, const Tensor &kl_row, double s, double nw2, double c_hard, double c_soft,
                      double inv_tau, bool first) {
    TORCH_CHECK(n_cols >= 1 && n_rows >= 1 && ld_s >= n_cols && ld_s <= INT32_MAX && ld_t >= n_cols && ld_t <= INT32_MAX && n_rows <= INT32_MAX &&
                v0 >= 0 && v0 + n_cols <= INT32_MAX && inv_tau > 0.0 && std::isfinite(inv_tau), "jlm.train_distill_dy: bad shape");
    const c10::hip::HIPGuard device_guard(ys.device().index());
    jlm_check(jlm_distill_dy(vptr<float>(ys, at::kFloat, span(n_rows, ld_s, n_cols), "ys"), (int)ld_s,
                             vptr<const float>(yt, at::kFloat, span(n_rows, ld_t, n_cols), "yt"), (int)ld_t, (int)n_cols, (int)v0, (int)n_rows,
                             vptr<const float>(run, at::kFloat, 6 * n_rows, "run"), vptr<const int>(target, at::kInt, n_rows, "target"),
                             vptr<float>(tgt_logit, at::kFloat, n_rows, "tgt_logit"), vptr<float>(kl_row, at::kFloat, n_rows, "kl_row"), (float)s,
                             (float)nw2, (float)c_hard, (float)c_soft, (float)inv_tau, first ? 1 : 0, stream_of(ys)),
              "jlm_distill_dy");
}

void train_distill_kl(const Tensor &kl_row, int64_t n_rows, const Tensor &kl_out, const Tensor &flag) {
    TORCH_CHECK(n_rows >= 1 && n_rows <= INT32_MAX, "jlm.train_distill_kl: bad shape");
    const c10::hip::HIPGuard device_guard(kl_row.device().index());
    jlm_check(jlm_distill_kl(vptr<const float>(kl_row, at::kFloat, n_rows, "kl_row"), (int)n_rows, vptr<double>(kl_out, at::kDouble, 1, "kl_out"),
                             vptr<int>(flag, at::kInt, 1, "flag"), stream_of(kl_row)),
              "jlm_distill_kl");
}

void train_scatter_rows(const Tensor &dx, int64_t ld_dx, int64_t col0, int64_t n_cols, int64_t width, const Tensor &ids_sorted, const Tensor &perm,
                        int64_t n, const Tensor &demb, int64_t ld, int64_t v_lo, int64_t v_hi, int64_t key, int64_t thr, double scale) {
    TORCH_CHECK(n >= 1 && n <= INT32_MAX && n_cols >= 1 && col0 >= 0 && col0 + n_cols <= width && ld_dx >= width && ld_dx <= INT32_MAX &&
                ld >= n_cols && ld <= INT32_MAX && v_lo >= 0 && v_hi > v_lo && v_hi <= INT32_MAX && thr >= 0 && thr <= (1 << 24),
                "jlm.train_scatter_rows: bad shape");
    const c10::hip::HIPGuard device_guard(demb.device().index());
    jlm_check(jlm_train_scatter_rows(vptr<const float>(dx, at::kFloat, span(n, ld_dx, width), "dx"), (int)ld_dx, (int)col0, (int)n_cols, (int)width,
                                     vptr<const int>(ids_sorted, at::kInt, n, "ids_sorted"), vptr<const long long>(perm, at::kLong, n, "perm"),
                                     (int)n, vptr<float>(demb, at::kFloat, span(v_hi - v_lo, ld, n_cols), "demb"), (int)ld, (int)v_lo, (int)v_hi,
                                     (uint64_t)key, (unsigned)thr, (float)scale, stream_of(demb)),
              "jlm_train_scatter_rows");
}

void train_adam(const Tensor &w, const Tensor &g, const Tensor &m, const Tensor &v, int64_t n, double lr_t, const OptTensor &flag) {
    TORCH_CHECK(n >= 4 && n % 4 == 0, "jlm.train_adam: n must be a positive multiple of 4");
    const c10::hip::HIPGuard device_guard(w.device().index());
    const bool has_flag = flag.has_value() && flag->defined();
    jlm_check(jlm_train_adam(vptr<float>(w, at::kFloat, n, "w"), vptr<const float>(g, at::kFloat, n, "g"), vptr<float>(m, at::kFloat, n, "m"),
                             vptr<float>(v, at::kFloat, n, "v"), (long long)n, (float)lr_t,
                             has_flag ? vptr<const int>(*flag, at::kInt, 1, "flag") : nullptr, stream_of(w)),
              "jlm_train_adam");
}

// ---- dynamic evaluation (jlm_amd/dyneval.py)
void train_gemm_splitk(const Tensor &A, int64_t sam, int64_t sak, const Tensor &B, int64_t sbk, int64_t sbn, const Tensor &C, int64_t ldc,
                       int64_t M, int64_t N, int64_t K, bool accumulate, const OptTensor &bias, int64_t kc, const Tensor &part) {
    TORCH_CHECK(M >= 1 && N >= 1 && K >= 1 && M <= INT32_MAX && N <= INT32_MAX && K <= INT32_MAX && ldc >= N && ldc <= INT32_MAX && sam >= 1 &&
                sak >= 1 && sbk >= 1 && sbn >= 1 && kc >= 16 && kc % 16 == 0 && kc <= INT32_MAX, "jlm.train_gemm_splitk: bad shape");
    TORCH_CHECK(part.defined() && part.is_contiguous() && part.numel() >= (K + kc - 1) / kc * M * N,
                "jlm.train_gemm_splitk: `part` holds fewer than ceil(K / kc) M N values");
    const c10::hip::HIPGuard device_guard(C.device().index());
    const bool has_bias = bias.has_value() && bias->defined();
    jlm_check(jlm_train_gemm_splitk(vptr<const float>(A, at::kFloat, (M - 1) * sam + (K - 1) * sak + 1, "A"), sam, sak,
                                    vptr<const float>(B, at::kFloat, (K - 1) * sbk + (N - 1) * sbn + 1, "B"), sbk, sbn,
                                    vptr<float>(C, at::kFloat, span(M, ldc, N), "C"), (int)ldc, (int)M, (int)N, (int)K, accumulate ? 1 : 0,
                                    has_bias ? vptr<const float>(*bias, at::kFloat, N, "bias") : nullptr, (int)kc,
                                    vptr<float>(part, at::kFloat, part.numel(), "part"), (long long)part.numel(), stream_of(C)),
              "jlm_train_gemm_splitk");
}

void dyneval_sqacc(const Tensor &ms, const Tensor &g, int64_t n, const OptTensor &flag) {
    TORCH_CHECK(n >= 4 && n % 4 == 0, "jlm.dyneval_sqacc: n must be a positive multiple of 4");
    const c10::hip::HIPGuard device_guard(ms.device().index());
    const bool has_flag = flag.has_value() && flag->defined();
    jlm_check(jlm_dyneval_sqacc(vptr<float>(ms, at::kFloat, n, "ms"), vptr<const float>(g, at::kFloat, n, "g"), (long long)n,
                                has_flag ? vptr<const int>(*flag, at::kInt, 1, "flag") : nullptr, stream_of(ms)),
              "jlm_dyneval_sqacc");
}

void dyneval_rms(const Tensor &ms, int64_t n, double inv_chunks, const Tensor &rms, int64_t n_real, const Tensor &partial,
                 const Tensor &mean_out) {
    TORCH_CHECK(n >= 4 && n % 4 == 0 && n_real >= 1 && n_real <= n && inv_chunks > 0.0 && std::isfinite(inv_chunks),
                "jlm.dyneval_rms: n must be a positive multiple of 4, 1 <= n_real <= n, inv_chunks > 0");
    const c10::hip::HIPGuard device_guard(ms.device().index());
    jlm_check(jlm_dyneval_rms(vptr<const float>(ms, at::kFloat, n, "ms"), (long long)n, (float)inv_chunks, vptr<float>(rms, at::kFloat, n, "rms"),
                              (long long)n_real, vptr<double>(partial, at::kDouble, JLM_DYNEVAL_MAX_BLOCKS, "partial"),
                              vptr<double>(mean_out, at::kDouble, 1, "mean_out"), stream_of(ms)),
              "jlm_dyneval_rms");
}

void dyneval_update(const Tensor &w, const Tensor &g, const Tensor &w0, const OptTensor &rms, int64_t n, double lr, double lam_scale, double eps,
                    const OptTensor &flag) {
    TORCH_CHECK(n >= 4 && n % 4 == 0, "jlm.dyneval_update: n must be a positive multiple of 4");
    const c10::hip::HIPGuard device_guard(w.device().index());
    const bool has_rms = rms.has_value() && rms->defined(), has_flag = flag.has_value() && flag->defined();
    jlm_check(jlm_dyneval_update(vptr<float>(w, at::kFloat, n, "w"), vptr<const float>(g, at::kFloat, n, "g"),
                                 vptr<const float>(w0, at::kFloat, n, "w0"), has_rms ? vptr<const float>(*rms, at::kFloat, n, "rms") : nullptr,
                                 (long long)n, lr, lam_scale, eps,
                                 has_flag ? vptr<const int>(*flag, at::kInt, 1, "flag") : nullptr, stream_of(w)),
              "jlm_dyneval_update");
}

// ---- fine-tuning the codebooks of a compressed model (jlm_amd/finetune.py)
void train_expand_codes(const Tensor &book, const Tensor &gid, const Tensor &w, int64_t n) {
    TORCH_CHECK(n >= 4 && n % 4 == 0, "jlm.train_expand_codes: n must be a positive multiple of 4");
    TORCH_CHECK(book.defined() && book.numel() >= 1 && book.numel() <= INT32_MAX, "jlm.train_expand_codes: an empty codebook buffer");
    const c10::hip::HIPGuard device_guard(w.device().index());
    jlm_check(jlm_train_expand_codes(vptr<const float>(book, at::kFloat, book.numel(), "book"), (int)book.numel(),
                                     vptr<const int>(gid, at::kInt, n, "gid"), vptr<float>(w, at::kFloat, n, "w"), (long long)n, stream_of(w)),
              "jlm_train_expand_codes");
}

void train_codebook_grad(const Tensor &g, const Tensor &order, const Tensor &chunks, int64_t n_chunks, int64_t n_groups, const Tensor &partial,
                         const Tensor &gbook) {
    TORCH_CHECK(n_chunks >= 0 && n_chunks <= INT32_MAX / 3 && n_groups >= 1 && n_groups <= INT32_MAX, "jlm.train_codebook_grad: bad shape");
    TORCH_CHECK(g.defined() && g.numel() >= 1 && order.defined(), "jlm.train_codebook_grad: g and order must be tensors");
    const c10::hip::HIPGuard device_guard(gbook.device().index());
    const int64_t n_order = order.numel();
    jlm_check(jlm_train_codebook_grad(vptr<const float>(g, at::kFloat, g.numel(), "g"), (long long)g.numel(),
                                      n_order ? vptr<const int>(order, at::kInt, n_order, "order") : nullptr, (long long)n_order,
                                      n_chunks ? vptr<const int>(chunks, at::kInt, 3 * n_chunks, "chunks") : nullptr, (int)n_chunks,
                                      (int)n_groups, n_chunks ? vptr<double>(partial, at::kDouble, n_chunks, "partial") : nullptr,
                                      vptr<float>(gbook, at::kFloat, n_groups, "gbook"), stream_of(gbook)),
              "jlm_train_codebook_grad");
}

int64_t abi_version() { return jlm_abi_version(); }
int64_t beam_step_max_cands(int64_t beam, int64_t n_frames, int64_t mode) { return jlm_beam_step_max_cands((int)beam, (int)n_frames, (int)mode); }

}  // namespace

TORCH_LIBRARY(jlm, m) {
    m.class_<JlmModel>("Model").def(
        torch::init<TDict, IDict, FDict, std::vector<Tensor>, std::vector<int64_t>, std::vector<Tensor>, std::vector<int64_t>,
                    std::vector<double>, std::vector<double>, std::vector<int64_t>, std::vector<int64_t>, std::vector<Tensor>,
                    std::vector<int64_t>, std::vector<double>, std::vector<double>, std::vector<double>, std::vector<int64_t>>());
    m.class_<JlmPlan>("Plan").def(torch::init<TDict, IDict>());
    m.def("decode_frames(__torch__.torch.classes.jlm.Model model, __torch__.torch.classes.jlm.Plan plan, int n_frames, int vs_max, "
          "int di_max, int dd_max, bool use_side, bool timed, int lse_cu_share_pct) -> int", decode_frames);
    m.def("decode_batch(__torch__.torch.classes.jlm.Model model, __torch__.torch.classes.jlm.Plan plan, Tensor host_ints, int head_end, "
          "Tensor? blk, int[] blk_src, int[] blk_dst, int[] blk_n, Tensor(a!) h_nodes, Tensor(b!) h_len, Tensor(c!) h_score, Tensor? h_nlive, "
          "int n_frames, int vs_max, int di_max, int dd_max, bool use_side, bool timed, int lse_cu_share_pct) -> int", decode_batch);
    m.def("frame_times(__torch__.torch.classes.jlm.Plan plan) -> Tensor", frame_times);
    m.def("lstm_step(Tensor h_in, Tensor c_in, int ld_state, Tensor(a!) h_out, Tensor(b!) c_out, Tensor? rows, Tensor prev, Tensor word, "
          "Tensor emb, int ld_emb, Tensor wt, Tensor bias, int kpad, int H, int E, int n_rows_max, Tensor? n_dev) -> ()", lstm_step);
    m.def("gemm_nt(Tensor A, int a_off, int lda, Tensor? a_rows, Tensor B, int ldb, Tensor? b_rows, Tensor(a!) C, int c_off, int ldc, "
          "Tensor? c_rows, Tensor? bias, int bias_off, int M, int N, int K, Tensor? m_dev) -> ()", gemm_nt);
    m.def("softmax_rows(Tensor y, Tensor(a!) pred, int ld, int n_rows, int n_cols, bool self_norm) -> ()", softmax_rows);
    m.def("pack_split_f16(Tensor src, int src_off, int rows, int k, int ld, float scale, Tensor(a!) dst, int dst_off, int ld_dst) -> ()",
          pack_split_f16);
    m.def("pack_split_f16_col(Tensor v, int v_off, int rows, float scale, Tensor(a!) dst, int ld_dst, int col) -> ()", pack_split_f16_col);
    m.def("pack_mixed(Tensor src, int src_off, int rows, int k, int ld, Tensor bias, int bias_off, float scale, float bias_scale, float s8, "
          "Tensor(a!) dst, int ld_dst) -> ()", pack_mixed);
    m.def("dequant_u8(Tensor code, int rows, int k, int ld_code, Tensor codebook, Tensor(a!) dst, int ld_dst) -> ()", dequant_u8);
    m.def("lse_probe(__torch__.torch.classes.jlm.Model model, Tensor rowlist, Tensor prev, Tensor word, int steps, int rows, Tensor(a!) h, "
          "Tensor(b!) c, Tensor(c!) T, Tensor? Tm, int ld_tm, int form, Tensor(d!) part, int max_parts) -> int", lse_probe);
    m.def("score_frames(__torch__.torch.classes.jlm.Model model, Tensor(a!) h0, Tensor(b!) c0, Tensor(c!) h1, Tensor(d!) c1, Tensor(e!)? T, "
          "Tensor(f!)? Tm, int ld_tm, Tensor(g!)? part, int max_parts, Tensor rows, Tensor prev0, Tensor word, Tensor target, Tensor n_live, "
          "int[] n_live_host, Tensor(h!) nll_seq, Tensor(i!)? nll_tok, Tensor(j!)? flags, int n_rows, int n_steps, bool timed) -> Tensor",
          score_frames);
    m.def("alt_frames(__torch__.torch.classes.jlm.Model model, __torch__.torch.classes.jlm.Plan plan, int rank, Tensor sent_off, "
          "Tensor sent_rows, Tensor depth, Tensor alt, Tensor(a!) h0, Tensor(b!) c0, Tensor(c!) h1, Tensor(d!) c1, Tensor(e!)? T, "
          "Tensor(f!)? Tm, int ld_tm, Tensor(g!)? part, int max_parts, Tensor rows, Tensor(k!) prev0, Tensor word, Tensor target, "
          "Tensor n_live, int[] n_live_host, Tensor(h!) nll_seq, Tensor(i!)? nll_tok, Tensor(j!)? flags, int n_rows, int n_steps, "
          "bool timed) -> Tensor",
          alt_frames);
    m.def("score_cache_frames(__torch__.torch.classes.jlm.Model model, Tensor(a!) h0, Tensor(b!) c0, Tensor(c!) h1, Tensor(d!) c1, Tensor(e!)? T, "
          "Tensor(f!)? Tm, int ld_tm, Tensor(g!)? part, int max_parts, Tensor rows, Tensor prev0, Tensor word, Tensor target, Tensor n_live, "
          "int[] n_live_host, Tensor(h!) nll_seq, Tensor(i!)? nll_tok, Tensor(j!)? flags, int n_rows, int n_steps, bool timed, "
          "Tensor(k!) hist, Tensor(l!) words, int cap, int pos0, Tensor first, Tensor len, int N, float[] thetas, Tensor(m!) lpc, "
          "Tensor(n!)? cache_flags) -> Tensor",
          score_cache_frames);
    m.def("score_memory_frames(__torch__.torch.classes.jlm.Model model, Tensor(a!) h0, Tensor(b!) c0, Tensor(c!) h1, Tensor(d!) c1, Tensor(e!)? T, "
          "Tensor(f!)? Tm, int ld_tm, Tensor(g!)? part, int max_parts, Tensor rows, Tensor prev0, Tensor word, Tensor target, Tensor n_live, "
          "int[] n_live_host, Tensor(h!) nll_seq, Tensor(i!)? nll_tok, Tensor(j!)? flags, int n_rows, int n_steps, bool timed, "
          "Tensor keys, Tensor key_words, int N, Tensor(k!) q_rows, Tensor(l!) q_words, Tensor len, float[] thetas, Tensor(m!) lpm, "
          "Tensor(n!) workspace, Tensor(o!)? mem_flags) -> Tensor",
          score_memory_frames);
    m.def("rank_rows(Tensor y, int ld, int n_cols, int n_rows, Tensor? n_dev, Tensor target, Tensor? ids, Tensor? lv_off, Tensor? lv_lo, "
          "Tensor? lv_hi, int n_levels, Tensor(a!) rank, Tensor(b!)? flags) -> ()",
          rank_rows);
    m.def("rank_frames(__torch__.torch.classes.jlm.Model model, Tensor(a!) h0, Tensor(b!) c0, Tensor(c!) h1, Tensor(d!) c1, Tensor(e!)? T, "
          "Tensor(f!) logits, int ld_logits, Tensor rows, Tensor prev0, Tensor word, Tensor target, Tensor n_live, int[] n_live_host, "
          "Tensor? ids, Tensor? lv_off, Tensor? lv_lo, Tensor? lv_hi, int n_levels, Tensor(g!) rank, Tensor(h!)? flags, int n_rows, "
          "int n_steps, bool timed) -> Tensor",
          rank_frames);
    m.def("rank_cache_frames(__torch__.torch.classes.jlm.Model model, Tensor(a!) h0, Tensor(b!) c0, Tensor(c!) h1, Tensor(d!) c1, Tensor(e!)? T, "
          "Tensor(f!) logits, int ld_logits, Tensor rows, Tensor prev0, Tensor word, Tensor target, Tensor n_live, int[] n_live_host, "
          "Tensor? ids, Tensor? lv_off, Tensor? lv_lo, Tensor? lv_hi, int n_levels, Tensor(g!) rank, Tensor(h!)? flags, int n_rows, "
          "int n_steps, bool timed, Tensor(i!) hist, Tensor(j!) words, int cap, int pos0, Tensor first, int N, float theta, float lam, "
          "Tensor(k!) s, int ld_s, int top_k, Tensor(l!)? top_ids, Tensor(m!)? top_nll, Tensor(n!)? cache_flags) -> Tensor",
          rank_cache_frames);
    m.def("predict_cache_rows(__torch__.torch.classes.jlm.Model model, Tensor h, Tensor(a!)? T, Tensor(b!) logits, int ld_logits, Tensor rows, "
          "Tensor hist, Tensor words, int cap, int pos, Tensor first, int N, float theta, float lam, Tensor(c!) s, int ld_s, int k, "
          "Tensor? mask, int ld_mask, int n_sets, int[] row_set, Tensor(d!) ids, Tensor(e!) nll, Tensor(f!)? flags, Tensor(g!)? cache_flags, "
          "int n_rows) -> ()",
          predict_cache_rows);
    m.def("rank_memory_frames(__torch__.torch.classes.jlm.Model model, Tensor(a!) h0, Tensor(b!) c0, Tensor(c!) h1, Tensor(d!) c1, Tensor(e!)? T, "
          "Tensor(f!) logits, int ld_logits, Tensor rows, Tensor prev0, Tensor word, Tensor target, Tensor n_live, int[] n_live_host, "
          "Tensor? ids, Tensor? lv_off, Tensor? lv_lo, Tensor? lv_hi, int n_levels, Tensor(g!) rank, Tensor(h!)? flags, int n_rows, "
          "int n_steps, bool timed, Tensor keys, Tensor key_words, int N, float theta, float lam, int K, Tensor(i!) s, int ld_s, "
          "Tensor(j!) ret_words, Tensor(k!) ret_idx, bool keep_idx, Tensor first, Tensor(l!) workspace, int top_k, Tensor(m!)? top_ids, "
          "Tensor(n!)? top_nll, Tensor(o!)? mem_flags) -> Tensor",
          rank_memory_frames);
    m.def("predict_memory_rows(__torch__.torch.classes.jlm.Model model, Tensor h, Tensor(a!)? T, Tensor(b!) logits, int ld_logits, Tensor rows, "
          "Tensor keys, Tensor key_words, int N, float theta, float lam, int K, Tensor(c!) s, int ld_s, Tensor(d!) ret_words, "
          "Tensor(e!)? ret_idx, Tensor first, Tensor(f!) workspace, int k, Tensor? mask, int ld_mask, int n_sets, int[] row_set, "
          "Tensor(g!) ids, Tensor(h!) nll, Tensor(i!)? flags, Tensor(j!)? mem_flags, int n_rows) -> ()",
          predict_memory_rows);
    m.def("sample_rows(Tensor y, int ld, int n_cols, int n_rows, Tensor? n_dev, float temperature, int seed, int step, Tensor? row_id, "
          "Tensor? forced, Tensor(a!)? done, int stop_id, bool self_norm, Tensor(b!) word, Tensor(c!) ids, Tensor(d!) nll, Tensor(e!)? flags) -> ()",
          sample_rows);
    m.def("generate_frames(__torch__.torch.classes.jlm.Model model, Tensor(a!) h0, Tensor(b!) c0, Tensor(c!) h1, Tensor(d!) c1, Tensor(e!)? T, "
          "Tensor(f!) logits, int ld_logits, Tensor rows, Tensor prev, Tensor prompt, Tensor n_live, int[] n_live_host, Tensor row_id, "
          "Tensor(g!) word, Tensor(h!)? done, int stop_id, float temperature, int seed, Tensor(i!) ids, Tensor(j!) nll, Tensor(k!)? flags, "
          "int n_rows, int n_prompt, int n_words, bool timed) -> Tensor",
          generate_frames);
    m.def("sample_rows_trunc(Tensor y, int ld, int n_cols, int n_rows, Tensor? n_dev, float temperature, int seed, int step, Tensor? row_id, "
          "Tensor? forced, Tensor(a!)? done, int stop_id, bool self_norm, int top_k, float top_p, Tensor(b!) word, Tensor(c!) ids, "
          "Tensor(d!) nll, Tensor(e!)? flags) -> ()",
          sample_rows_trunc);
    m.def("generate_frames_trunc(__torch__.torch.classes.jlm.Model model, Tensor(a!) h0, Tensor(b!) c0, Tensor(c!) h1, Tensor(d!) c1, "
          "Tensor(e!)? T, Tensor(f!) logits, int ld_logits, Tensor rows, Tensor prev, Tensor prompt, Tensor n_live, int[] n_live_host, "
          "Tensor row_id, Tensor(g!) word, Tensor(h!)? done, int stop_id, float temperature, int seed, Tensor(i!) ids, Tensor(j!) nll, "
          "Tensor(k!)? flags, int n_rows, int n_prompt, int n_words, bool timed, int top_k, float top_p) -> Tensor",
          generate_frames_trunc);
    m.def("topk_rows(Tensor y, int ld, int n_cols, int n_rows, int k, bool self_norm, Tensor(a!) ids, Tensor(b!) nll, int ld_out, "
          "Tensor(c!)? flags) -> ()",
          topk_rows);
    m.def("memory_topk(Tensor keys, Tensor key_words, int N, int H, bool split, float h_scale, Tensor q_rows, int n_rows, float theta, int K, "
          "Tensor(a!) s, int ld_s, Tensor(b!) ret_words, Tensor(c!) ret_idx, Tensor(d!) workspace, Tensor(e!)? flags) -> ()",
          memory_topk);
    m.def("beam_merge(Tensor cand_ids, Tensor cand_nll, int beam, int n_prompts, bool first, int stop_id, Tensor(a!) word, Tensor(b!) prev, "
          "Tensor(c!) score, Tensor(d!) finished, Tensor(e!) bp_parent, Tensor(f!) bp_word, Tensor(g!) bp_nll) -> ()",
          beam_merge);
    m.def("complete_frames(__torch__.torch.classes.jlm.Model model, Tensor(a!) h0, Tensor(b!) c0, Tensor(c!) h1, Tensor(d!) c1, Tensor(e!)? T, "
          "Tensor(f!) logits, int ld_logits, Tensor rows, Tensor prev, Tensor prompt, Tensor n_live, int[] n_live_host, Tensor(g!) cand_ids, "
          "Tensor(h!) cand_nll, Tensor(i!) word, Tensor(j!) prev_row, Tensor(k!) score, Tensor(l!) finished, int stop_id, Tensor(m!) bp_parent, "
          "Tensor(n!) bp_word, Tensor(o!) bp_nll, Tensor(p!)? flags, int n_prompts, int beam, int n_prompt, int n_words, bool timed) -> Tensor",
          complete_frames);
    m.def("topk_rows_masked(Tensor y, int ld, int n_cols, int n_rows, int k, bool self_norm, Tensor mask, int ld_mask, int n_sets, "
          "int[] row_set, Tensor(a!) ids, Tensor(b!) nll, int ld_out, Tensor(c!)? flags) -> ()",
          topk_rows_masked);
    m.def("complete_frames_masked(__torch__.torch.classes.jlm.Model model, Tensor(a!) h0, Tensor(b!) c0, Tensor(c!) h1, Tensor(d!) c1, "
          "Tensor(e!)? T, Tensor(f!) logits, int ld_logits, Tensor rows, Tensor prev, Tensor prompt, Tensor n_live, int[] n_live_host, "
          "Tensor(g!) cand_ids, Tensor(h!) cand_nll, Tensor(i!) word, Tensor(j!) prev_row, Tensor(k!) score, Tensor(l!) finished, int stop_id, "
          "Tensor(m!) bp_parent, Tensor(n!) bp_word, Tensor(o!) bp_nll, Tensor(p!)? flags, int n_prompts, int beam, int n_prompt, int n_words, "
          "bool timed, Tensor? mask, int ld_mask, int n_sets, int[] prompt_set) -> Tensor",
          complete_frames_masked);
    m.def("complete_frames_ngram(__torch__.torch.classes.jlm.Model model, Tensor(a!) h0, Tensor(b!) c0, Tensor(c!) h1, Tensor(d!) c1, "
          "Tensor(e!)? T, Tensor(f!) logits, int ld_logits, Tensor rows, Tensor prev, Tensor prompt, Tensor n_live, int[] n_live_host, "
          "Tensor(g!) cand_ids, Tensor(h!) cand_nll, Tensor(i!) word, Tensor(j!) prev_row, Tensor(k!) score, Tensor(l!) finished, int stop_id, "
          "Tensor(m!) bp_parent, Tensor(n!) bp_word, Tensor(o!) bp_nll, Tensor(p!)? flags, int n_prompts, int beam, int n_prompt, int n_words, "
          "bool timed, Tensor? mask, int ld_mask, int n_sets, int[] prompt_set, Tensor[] table, int[] sizes, int order, float lam, "
          "Tensor(q!) hist0, Tensor(r!) hist1, Tensor(s!)? ngram_flags) -> Tensor",
          complete_frames_ngram);
    m.def("rank_ngram_frames(__torch__.torch.classes.jlm.Model model, Tensor(a!) h0, Tensor(b!) c0, Tensor(c!) h1, Tensor(d!) c1, Tensor(e!)? T, "
          "Tensor(f!) logits, int ld_logits, Tensor rows, Tensor prev0, Tensor word, Tensor target, Tensor n_live, int[] n_live_host, "
          "Tensor? ids, Tensor? lv_off, Tensor? lv_lo, Tensor? lv_hi, int n_levels, Tensor(g!) rank, Tensor(h!)? flags, int n_rows, "
          "int n_steps, bool timed, Tensor[] table, int[] sizes, int order, float lam, Tensor hist, int top_k, Tensor(i!)? top_ids, "
          "Tensor(j!)? top_nll, Tensor(k!)? ngram_flags) -> Tensor",
          rank_ngram_frames);
    m.def("kmeans1d(Tensor x, int bit, int seed, int max_iter, float tol, Tensor(a!) code, Tensor(b!) codebook, Tensor(c!) scratch, int grid, "
          "bool timed) -> Tensor",
          kmeans1d);
    m.def("train_gemm(Tensor A, int sam, int sak, Tensor B, int sbk, int sbn, Tensor(a!) C, int ldc, int M, int N, int K, bool accumulate, "
          "Tensor? bias) -> ()", train_gemm);
    m.def("train_embed_rows(Tensor emb, int ld_emb, int V, Tensor ids, int n_rows, int E, Tensor(a!) x, int key, int thr, float scale) -> ()",
          train_embed_rows);
    m.def("train_cell_fwd(Tensor(a!) z, Tensor c_prev, Tensor(b!) c, Tensor(c!) h, Tensor(d!) r, int B, int H, int row0, int key, int thr, "
          "float scale) -> ()", train_cell_fwd);
    m.def("train_cell_bwd(Tensor gates, Tensor c, Tensor c_prev, Tensor dr, Tensor? dh_next, Tensor(a!) dc, Tensor(b!) dz, int B, int H, "
          "int row0, int key, int thr, float scale) -> ()", train_cell_bwd);
    m.def("train_lse_update(Tensor y, int ld, int n_cols, int n_rows, Tensor(a!) run_m, Tensor(b!) run_s, bool first) -> ()", train_lse_update);
    m.def("train_dy(Tensor(a!) y, int ld, int n_cols, int v0, int n_rows, Tensor run_m, Tensor run_s, Tensor target, Tensor(b!) tgt_logit, "
          "float s, float nw2) -> ()", train_dy);
    m.def("train_colsum(Tensor a, int ld, int n_rows, int n_cols, Tensor(a!) out, bool accumulate) -> ()", train_colsum);
    m.def("train_ce(Tensor run_m, Tensor run_s, Tensor tgt_logit, int n_rows, float nw, Tensor(a!) ce_out, Tensor(b!) flag) -> ()", train_ce);
    m.def("train_distill_lse_update(Tensor ys, int ld_s, Tensor yt, int ld_t, int n_cols, int n_rows, float inv_tau, Tensor(a!) run, "
          "bool first) -> ()", train_distill_lse_update);
    m.def("train_distill_dy(Tensor(a!) ys, int ld_s, Tensor yt, int ld_t, int n_cols, int v0, int n_rows, Tensor run, Tensor target, "
          "Tensor(b!) tgt_logit, Tensor(c!) kl_row, float s, float nw2, float c_hard, float c_soft, float inv_tau, bool first) -> ()",
          train_distill_dy);
    m.def("train_distill_kl(Tensor kl_row, int n_rows, Tensor(a!) kl_out, Tensor(b!) flag) -> ()", train_distill_kl);
    m.def("train_scatter_rows(Tensor dx, int ld_dx, int col0, int n_cols, int width, Tensor ids_sorted, Tensor perm, int n, Tensor(a!) demb, "
          "int ld, int v_lo, int v_hi, int key, int thr, float scale) -> ()", train_scatter_rows);
    m.def("train_adam(Tensor(a!) w, Tensor g, Tensor(b!) m, Tensor(c!) v, int n, float lr_t, Tensor? flag) -> ()", train_adam);
    m.def("train_gemm_splitk(Tensor A, int sam, int sak, Tensor B, int sbk, int sbn, Tensor(a!) C, int ldc, int M, int N, int K, bool accumulate, "
          "Tensor? bias, int kc, Tensor(b!) part) -> ()", train_gemm_splitk);
    m.def("dyneval_sqacc(Tensor(a!) ms, Tensor g, int n, Tensor? flag) -> ()", dyneval_sqacc);
    m.def("dyneval_rms(Tensor ms, int n, float inv_chunks, Tensor(a!) rms, int n_real, Tensor(b!) partial, Tensor(c!) mean_out) -> ()", dyneval_rms);
    m.def("dyneval_update(Tensor(a!) w, Tensor g, Tensor w0, Tensor? rms, int n, float lr, float lam_scale, float eps, Tensor? flag) -> ()",
          dyneval_update);
    m.def("train_expand_codes(Tensor book, Tensor gid, Tensor(a!) w, int n) -> ()", train_expand_codes);
    m.def("train_codebook_grad(Tensor g, Tensor order, Tensor chunks, int n_chunks, int n_groups, Tensor(a!) partial, Tensor(b!) gbook) -> ()",
          train_codebook_grad);
    m.def("prime_frames(__torch__.torch.classes.jlm.Model model, Tensor(a!) h0, Tensor(b!) c0, Tensor(c!) h1, Tensor(d!) c1, Tensor rows, "
          "Tensor prev, Tensor word, Tensor n_live, int[] n_live_host, int n_rows, int n_steps) -> ()", prime_frames);
    m.def("seed_context(__torch__.torch.classes.jlm.Plan plan, Tensor src_h, Tensor src_c, Tensor last, Tensor has, Tensor idx) -> ()",
          seed_context);
    m.def("prime_cache_frames(__torch__.torch.classes.jlm.Model model, Tensor(a!) h0, Tensor(b!) c0, Tensor(c!) h1, Tensor(d!) c1, Tensor rows, "
          "Tensor prev, Tensor word, Tensor n_live, int[] n_live_host, int n_rows, int n_steps, Tensor target, Tensor(e!) hist, "
          "Tensor(f!) words, int cap) -> ()", prime_cache_frames);
    m.def("seed_cache(__torch__.torch.classes.jlm.Plan plan, Tensor hist, Tensor words, Tensor count, Tensor idx, Tensor(a!) s, int cap, int N, "
          "float theta, float lam) -> ()", seed_cache);
    m.def("clear_cache(__torch__.torch.classes.jlm.Plan plan) -> ()", clear_cache);
    m.def("seed_ngram(__torch__.torch.classes.jlm.Plan plan, Tensor keys, Tensor vals, Tensor root_hist, int log2cap, int max_probe, int order, "
          "float lam) -> ()", seed_ngram);
    m.def("clear_ngram(__torch__.torch.classes.jlm.Plan plan) -> ()", clear_ngram);
    m.def("seed_memory(__torch__.torch.classes.jlm.Plan plan, Tensor keys, Tensor key_words, int N, int H, float theta, float lam, int K, "
          "Tensor(a!) q_rows, Tensor(b!) s, Tensor(c!) ret_words, Tensor(d!) workspace, Tensor(e!) flags) -> ()", seed_memory);
    m.def("clear_memory(__torch__.torch.classes.jlm.Plan plan) -> ()", clear_memory);
    m.def("tail_predict(__torch__.torch.classes.jlm.Model model, __torch__.torch.classes.jlm.Plan plan, Tensor ids, Tensor sp_off, "
          "Tensor sp_frame, Tensor sp_lo, Tensor sp_hi, int n_out, int chunk, Tensor(a!) out_score, Tensor(b!) out_row, Tensor(c!) out_word, "
          "Tensor(d!) out_nodes, Tensor(e!) out_len, int stride) -> ()", tail_predict);
    m.def("abi_version() -> int", abi_version);
    m.def("beam_step_max_cands(int beam, int n_frames, int mode) -> int", beam_step_max_cands);
}
