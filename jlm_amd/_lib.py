"""ctypes binding of libjlm_hip.so (C ABI declared in include/jlm_hip.h).

The product path has no CPU fallback: :func:`lib` raises if the shared library
has not been built (``python -c 'import __graft_entry__ as g; g.build()'``) and
:func:`require_gpu` raises if no MI355X is visible.
"""
import ctypes
import os
from ctypes import POINTER, Structure, c_char_p, c_double, c_float, c_int, c_longlong, c_size_t, c_uint, c_uint64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
# JLM_HIP_LIB: developer override used by tools/ab_lib.sh to A/B two builds of the same ABI
LIB_PATH = os.environ.get("JLM_HIP_LIB") or os.path.join(_HERE, "csrc", "libjlm_hip.so")
HOST_LIB_PATH = os.path.join(_HERE, "csrc", "libjlm_host.so")

JLM_MAX_SEGMENTS = 8


class Segment(Structure):
    _fields_ = [("v_start", c_int), ("v_end", c_int), ("k", c_int), ("t_off", c_int),
                ("B", c_void_p), ("ldb", c_int)]


class Lattice(Structure):
    _fields_ = [("n_sent", c_int), ("beam", c_int), ("n_frames", c_int),
                ("sent_len", c_void_p), ("end_off", c_void_p),
                ("node_start", c_void_p), ("node_word", c_void_p)]


class BeamState(Structure):
    _fields_ = [("score", c_void_p), ("lse", c_void_p), ("ysum", c_void_p),
                ("bp", c_void_p), ("node", c_void_p), ("word", c_void_p),
                ("cnt", c_void_p), ("live", c_void_p), ("n_live", c_void_p),
                ("edge", c_void_p),
                ("live_base", c_void_p), ("lse_part", c_void_p), ("ld_part", c_int), ("n_parts", c_int), ("flags", c_void_p)]


class DecodeModel(Structure):
    """jlm_decode_model (include/jlm_hip.h)."""
    _fields_ = [("segs", POINTER(Segment)), ("n_segs", c_int), ("b2", c_void_p), ("H", c_int), ("ldt", c_int),
                ("untied", c_int), ("self_norm", c_int), ("split_lstm", c_int),
                ("emb", c_void_p), ("ld_emb", c_int), ("wt", c_void_p), ("gate_bias", c_void_p), ("kpad", c_int), ("E", c_int),
                ("gate_descale", c_float), ("h_scale", c_float),
                ("wt8", c_void_p), ("xgate8", c_void_p), ("untied_split", c_void_p), ("untied_descale", c_float), ("lse_fixed_ref", c_int),
                ("pmt", c_void_p), ("pmt_split", c_void_p), ("n_t", c_int), ("t_descale", c_float),
                ("split_segs", POINTER(Segment)), ("split_t_scale", POINTER(c_float)), ("split_descale", POINTER(c_float)),
                ("split_bias_col", POINTER(c_int)),
                ("mixed_segs", POINTER(Segment)), ("mixed_t_scale", POINTER(c_float)), ("mixed_descale", POINTER(c_float)),
                ("mixed_s8", POINTER(c_float)), ("mixed_bias2", c_void_p), ("mixed_head_split", POINTER(c_int))]


class DecodePlan(Structure):
    """jlm_decode_plan (include/jlm_hip.h)."""
    _fields_ = [("kind", c_int), ("max_cands", c_int), ("h", c_void_p), ("c", c_void_p), ("T", c_void_p),
                ("g0", c_void_p), ("cidx", c_void_p), ("sidx", c_void_p),
                ("sg_word", c_void_p), ("sg_off", c_void_p), ("sg_node", c_void_p), ("edge", c_void_p),
                ("vs_words", c_void_p), ("vs_off", c_void_p), ("vs_max", c_int),
                ("di_words", c_void_p), ("di_off", c_void_p), ("di_idx", c_void_p), ("di_max", c_int),
                ("dd_words", c_void_p), ("dd_off", c_void_p), ("dd_max", c_int),
                ("run_max", c_void_p), ("run_sum", c_void_p), ("part", c_void_p), ("max_parts", c_int), ("lse_cu_share_pct", c_int),
                ("out_nodes", c_void_p), ("out_len", c_void_p), ("out_score", c_void_p), ("stride", c_int),
                ("di_wwords", c_void_p), ("sg_wword", c_void_p), ("Tm", c_void_p), ("ld_tm", c_int),
                ("ctx_prev", c_void_p), ("ctx_word", c_void_p), ("cache", c_void_p), ("ngram", c_void_p), ("memory", c_void_p)]


class DecodeMemory(Structure):
    """jlm_decode_memory (include/jlm_hip.h)."""
    _fields_ = [("keys", c_void_p), ("key_words", c_void_p), ("N", c_int), ("K", c_int), ("theta", c_float), ("lam", c_float),
                ("q_rows", c_void_p), ("s", c_void_p), ("ld_s", c_int), ("ret_words", c_void_p), ("workspace", c_void_p),
                ("workspace_bytes", c_size_t), ("flags", c_void_p)]



class ScorePlan(Structure):
    """jlm_score_plan (include/jlm_hip.h)."""
    _fields_ = [("n_rows", c_int), ("n_steps", c_int), ("h", c_void_p * 2), ("c", c_void_p * 2), ("T", c_void_p),
                ("Tm", c_void_p), ("ld_tm", c_int), ("part", c_void_p), ("max_parts", c_int),
                ("rows", c_void_p), ("prev0", c_void_p), ("word", c_void_p), ("target", c_void_p),
                ("n_live", c_void_p), ("n_live_host", POINTER(c_int)),
                ("nll_seq", c_void_p), ("nll_tok", c_void_p), ("flags", c_void_p)]


class AltPlan(Structure):
    """jlm_alt_plan (include/jlm_hip.h)."""
    _fields_ = [("n_sent", c_int), ("beam", c_int), ("n_frames", c_int), ("rank", c_int), ("h", c_void_p), ("c", c_void_p),
                ("T", c_void_p), ("score", c_void_p), ("lse", c_void_p), ("bp", c_void_p), ("sent_len", c_void_p),
                ("sent_off", c_void_p), ("sent_rows", c_void_p), ("depth", c_void_p), ("alt", c_void_p), ("prev0", c_void_p)]


class GeneratePlan(Structure):
    """jlm_generate_plan (include/jlm_hip.h)."""
    _fields_ = [("n_rows", c_int), ("n_prompt", c_int), ("n_words", c_int), ("h", c_void_p * 2), ("c", c_void_p * 2), ("T", c_void_p),
                ("logits", c_void_p), ("ld_logits", c_int), ("rows", c_void_p), ("prev", c_void_p), ("prompt", c_void_p),
                ("n_live", c_void_p), ("n_live_host", POINTER(c_int)), ("row_id", c_void_p), ("word", c_void_p), ("done", c_void_p),
                ("stop_id", c_int), ("temperature", c_double), ("seed", c_uint64), ("ids", c_void_p), ("nll", c_void_p),
                ("flags", c_void_p)]


class RankPlan(Structure):
    """jlm_rank_plan (include/jlm_hip.h)."""
    _fields_ = [("n_rows", c_int), ("n_steps", c_int), ("h", c_void_p * 2), ("c", c_void_p * 2), ("T", c_void_p),
                ("logits", c_void_p), ("ld_logits", c_int), ("rows", c_void_p), ("prev0", c_void_p), ("word", c_void_p),
                ("target", c_void_p), ("n_live", c_void_p), ("n_live_host", POINTER(c_int)), ("ids", c_void_p), ("n_ids", c_int),
                ("lv_off", c_void_p), ("lv_lo", c_void_p), ("lv_hi", c_void_p), ("n_levels", c_int), ("rank", c_void_p),
                ("flags", c_void_p)]


class CachePlan(Structure):
    """jlm_cache_plan (include/jlm_hip.h)."""
    _fields_ = [("hist", c_void_p), ("words", c_void_p), ("cap", c_int), ("pos0", c_int), ("first", c_void_p), ("len", c_void_p),
                ("N", c_int), ("thetas", POINTER(c_float)), ("n_theta", c_int), ("lpc", c_void_p), ("flags", c_void_p)]


class MemoryPlan(Structure):
    """jlm_memory_plan (include/jlm_hip.h)."""
    _fields_ = [("keys", c_void_p), ("key_words", c_void_p), ("N", c_int), ("q_rows", c_void_p), ("q_words", c_void_p), ("len", c_void_p),
                ("thetas", POINTER(c_float)), ("n_theta", c_int), ("lpm", c_void_p), ("workspace", c_void_p), ("workspace_bytes", c_size_t),
                ("flags", c_void_p)]


class CacheMixPlan(Structure):
    """jlm_cache_mix_plan (include/jlm_hip.h)."""
    _fields_ = [("hist", c_void_p), ("words", c_void_p), ("cap", c_int), ("pos0", c_int), ("first", c_void_p), ("N", c_int),
                ("theta", c_float), ("lam", c_float), ("s", c_void_p), ("ld_s", c_int), ("top_k", c_int), ("top_ids", c_void_p),
                ("top_nll", c_void_p), ("flags", c_void_p)]


class PredictCachePlan(Structure):
    """jlm_predict_cache_plan (include/jlm_hip.h)."""
    _fields_ = [("n_rows", c_int), ("h", c_void_p), ("T", c_void_p), ("logits", c_void_p), ("ld_logits", c_int), ("rows", c_void_p),
                ("hist", c_void_p), ("words", c_void_p), ("cap", c_int), ("pos", c_int), ("first", c_void_p), ("N", c_int),
                ("theta", c_float), ("lam", c_float), ("s", c_void_p), ("ld_s", c_int), ("k", c_int), ("mask", c_void_p),
                ("ld_mask", c_int), ("n_sets", c_int), ("row_set", c_void_p), ("ids", c_void_p), ("nll", c_void_p), ("flags", c_void_p),
                ("cache_flags", c_void_p)]


class MemoryMixPlan(Structure):
    """jlm_memory_mix_plan (include/jlm_hip.h)."""
    _fields_ = [("keys", c_void_p), ("key_words", c_void_p), ("N", c_int), ("theta", c_float), ("lam", c_float), ("K", c_int),
                ("s", c_void_p), ("ld_s", c_int), ("ret_words", c_void_p), ("ret_idx", c_void_p), ("keep_idx", c_int), ("first", c_void_p),
                ("workspace", c_void_p), ("workspace_bytes", c_size_t), ("top_k", c_int), ("top_ids", c_void_p), ("top_nll", c_void_p),
                ("flags", c_void_p)]


class PredictMemoryPlan(Structure):
    """jlm_predict_memory_plan (include/jlm_hip.h)."""
    _fields_ = [("n_rows", c_int), ("h", c_void_p), ("T", c_void_p), ("logits", c_void_p), ("ld_logits", c_int), ("rows", c_void_p),
                ("keys", c_void_p), ("key_words", c_void_p), ("N", c_int), ("theta", c_float), ("lam", c_float), ("K", c_int),
                ("s", c_void_p), ("ld_s", c_int), ("ret_words", c_void_p), ("ret_idx", c_void_p), ("first", c_void_p),
                ("workspace", c_void_p), ("workspace_bytes", c_size_t), ("k", c_int), ("mask", c_void_p), ("ld_mask", c_int),
                ("n_sets", c_int), ("row_set", c_void_p), ("ids", c_void_p), ("nll", c_void_p), ("flags", c_void_p),
                ("memory_flags", c_void_p)]


class NgramRows(Structure):
    """jlm_ngram_rows (include/jlm_hip.h)."""
    _fields_ = [("uni_lp", c_void_p), ("uni_bow", c_void_p), ("bi_off", c_void_p), ("bi_w", c_void_p), ("bi_lp", c_void_p), ("n_bi", c_int),
                ("tri_off", c_void_p), ("tri_w", c_void_p), ("tri_lp", c_void_p), ("tri_bow", c_void_p), ("n_tri", c_int), ("n_ctx", c_int),
                ("ctx_keys", c_void_p), ("ctx_vals", c_void_p), ("log2cap", c_int), ("max_probe", c_int)]


class NgramMixPlan(Structure):
    """jlm_ngram_mix_plan (include/jlm_hip.h)."""
    _fields_ = [("table", POINTER(NgramRows)), ("order", c_int), ("lam", c_float), ("hist", c_void_p), ("top_k", c_int),
                ("top_ids", c_void_p), ("top_nll", c_void_p), ("flags", c_void_p)]


class CompleteNgramPlan(Structure):
    """jlm_complete_ngram_plan (include/jlm_hip.h)."""
    _fields_ = [("table", POINTER(NgramRows)), ("order", c_int), ("lam", c_float), ("hist", c_void_p * 2), ("flags", c_void_p)]


class PrimePlan(Structure):
    """jlm_prime_plan (include/jlm_hip.h)."""
    _fields_ = [("n_rows", c_int), ("n_steps", c_int), ("h", c_void_p * 2), ("c", c_void_p * 2), ("rows", c_void_p), ("prev", c_void_p),
                ("word", c_void_p), ("n_live", c_void_p), ("n_live_host", POINTER(c_int))]


class CompletePlan(Structure):
    """jlm_complete_plan (include/jlm_hip.h)."""
    _fields_ = [("n_prompts", c_int), ("beam", c_int), ("n_prompt", c_int), ("n_words", c_int), ("h", c_void_p * 2), ("c", c_void_p * 2),
                ("T", c_void_p), ("logits", c_void_p), ("ld_logits", c_int), ("rows", c_void_p), ("prev", c_void_p), ("prompt", c_void_p),
                ("n_live", c_void_p), ("n_live_host", POINTER(c_int)), ("cand_ids", c_void_p), ("cand_nll", c_void_p),
                ("word", c_void_p), ("prev_row", c_void_p), ("score", c_void_p), ("finished", c_void_p), ("stop_id", c_int),
                ("bp_parent", c_void_p), ("bp_word", c_void_p), ("bp_nll", c_void_p), ("flags", c_void_p)]


P = c_void_p
_SIGS = {
    "jlm_abi_version": ([], c_int),
    "jlm_device_arch": ([c_int, c_char_p, c_int], c_int),
    "jlm_lstm_step": ([P, P, c_int, P, P, P, P, P, P, c_int, P, P, c_int, c_int, c_int, c_int, P, P], c_int),
    "jlm_gemm_nt": ([P, c_int, P, P, c_int, P, P, c_int, P, P, c_int, c_int, c_int, P, P], c_int),
    "jlm_vocab_lse_partials": ([P, c_int, c_int, c_int, P, c_int, P, P, P, c_int, c_int, c_int, P, P], c_int),
    "jlm_lse_combine": ([P, c_int, c_int, P, P, c_int, P, P], c_int),
    "jlm_vocab_lse_stationary": ([POINTER(Segment), c_int, P, P, c_int, P, P, c_int, c_int, c_int, P, P], c_int),
    "jlm_pack_split_f16": ([P, c_int, c_int, c_int, c_float, P, c_int, P], c_int),
    "jlm_lstm_step_xg": ([P, P, c_int, P, P, P, P, P, P, P, c_int, c_float, c_float, P, c_int, P, P], c_int),
    "jlm_lstm_step_form": ([c_int, c_int, c_int, c_int], c_int),
    "jlm_vocab_lse_partials_split": ([P, c_int, c_int, c_int, P, c_int, P, P, c_float, P, c_int, c_int, c_int, P, P], c_int),
    "jlm_gemm_nt_split": ([P, c_int, P, P, c_int, P, P, c_int, P, P, c_float, c_int, c_int, c_int, P, P], c_int),
    "jlm_dequant_u8": ([P, c_int, c_int, c_int, P, c_int, P, c_int, P], c_int),
    "jlm_pack_split_f16_col": ([P, c_int, c_float, P, c_int, c_int, P], c_int),
    "jlm_vocab_lse_split": ([POINTER(Segment), POINTER(c_float), POINTER(c_float), POINTER(c_int), c_int, P, P, c_int, P, P,
                             c_int, c_int, c_int, P, P], c_int),
    "jlm_edge_logits": ([POINTER(Segment), c_int, P, P, c_int, P, P, P, P, P, P, c_int, P, P, c_int, c_int, P], c_int),
    "jlm_wordlist_lse": ([POINTER(Segment), c_int, P, P, c_int, P, P, P, P, P, P, c_int, P, P, P, c_int, c_int, c_int, P],
                         c_int),
    "jlm_edge_logits_perm": ([POINTER(Segment), c_int, P, P, c_int, P, P, P, P, P, P, P, c_int, P, P, c_int, c_int, P], c_int),
    "jlm_wordlist_lse_perm": ([POINTER(Segment), c_int, P, P, c_int, P, P, P, P, P, P, P, c_int, P, P, P, c_int, c_int, c_int, P],
                              c_int),
    "jlm_wordlist_lse_split": ([POINTER(Segment), c_float, c_float, P, P, c_int, P, P, P, P, P, P, c_int, c_int, P, P, P,
                               c_int, c_int, c_int, P], c_int),
    "jlm_wordlist_merge_split": ([POINTER(Segment), c_float, c_float, P, P, c_int, P, c_int, c_int, c_int, P, P, c_int, c_int,
                                 P, P, P, P], c_int),
    "jlm_beam_step": ([POINTER(Lattice), POINTER(BeamState), c_int, c_int, c_int, P], c_int),
    "jlm_beam_step_max_cands": ([c_int, c_int, c_int], c_int),
    "jlm_beam_step_lds_bytes": ([c_int, c_int, c_int, c_int], c_int),
    "jlm_vocab_lse_mixed_lds_bytes": ([POINTER(Segment), c_int], c_int),
    "jlm_pack_mixed": ([P, c_int, c_int, c_int, P, c_float, c_float, c_float, P, c_int, P], c_int),
    "jlm_vocab_lse_hybrid": ([POINTER(Segment), POINTER(c_float), POINTER(c_float), POINTER(c_int), POINTER(Segment), POINTER(c_float),
                              POINTER(c_float), POINTER(c_int), c_int, P, P, c_int, P, c_int, P, P, c_int, c_int, c_int, P, P], c_int),
    "jlm_mixed_t_stride": ([POINTER(Segment), c_int], c_int),
    "jlm_pack_t_mixed": ([POINTER(Segment), POINTER(c_float), c_int, P, c_int, P, c_int, P, P, c_int, P], c_int),
    "jlm_pack_t_mixed6": ([POINTER(Segment), POINTER(c_float), c_int, P, c_int, P, c_int, P, P, c_int, P], c_int),
    "jlm_vocab_lse_mixed": ([POINTER(Segment), POINTER(c_float), POINTER(c_float), P, c_int, P, c_int, P, c_int, c_int, c_int, P, P],
                            c_int),
    "jlm_pack_edge_mx6": ([POINTER(Segment), c_int, P, POINTER(Segment), POINTER(c_float), c_int, P, c_int, P, P, P, P, P, P, c_int, P, P,
                           c_int, c_int, P, P, c_int, P, c_int, P], c_int),
    "jlm_pack_edge_mx6_lds_bytes": ([c_int], c_int),
    "jlm_backtrace": ([POINTER(Lattice), POINTER(BeamState), P, P, P, c_int, P], c_int),
    "jlm_vocab_lse_mixed_fr": ([POINTER(Segment), POINTER(c_float), POINTER(c_float), P, c_int, P, c_int, P, c_int, c_int, c_int, P, P],
                            c_int),
    "jlm_softmax_rows": ([P, P, c_int, c_int, c_int, c_int, P], c_int),
    "jlm_decode_frames": ([POINTER(DecodeModel), POINTER(DecodePlan), POINTER(Lattice), POINTER(BeamState), P, P, P], c_int),
    "jlm_lse_probe": ([POINTER(DecodeModel), P, P, P, c_int, c_int, P, P, P, P, c_int, c_int, P, c_int, P], c_int),
    "jlm_score_frames": ([POINTER(DecodeModel), POINTER(ScorePlan), P, P], c_int),
    "jlm_score_fold": ([POINTER(Segment), c_int, P, P, c_int, P, c_int, c_int, c_int, P, P, c_int, P, P, P, P], c_int),
    "jlm_sample_rows": ([P, c_int, c_int, c_int, P, c_double, c_uint64, c_int, P, P, P, c_int, c_int, P, P, P, P, P], c_int),
    "jlm_generate_frames": ([POINTER(DecodeModel), POINTER(GeneratePlan), P, P], c_int),
    "jlm_sample_rows_trunc": ([P, c_int, c_int, c_int, P, c_double, c_uint64, c_int, P, P, P, c_int, c_int, c_int, c_double, P, P, P, P, P],
                              c_int),
    "jlm_generate_frames_trunc": ([POINTER(DecodeModel), POINTER(GeneratePlan), c_int, c_double, P, P], c_int),
    "jlm_topk_rows": ([P, c_int, c_int, c_int, c_int, c_int, P, P, c_int, P, P], c_int),
    "jlm_beam_merge": ([P, P, c_int, c_int, c_int, c_int, P, P, P, P, P, P, P, P], c_int),
    "jlm_complete_frames": ([POINTER(DecodeModel), POINTER(CompletePlan), P, P], c_int),
    "jlm_topk_rows_masked": ([P, c_int, c_int, c_int, c_int, c_int, P, c_int, c_int, P, P, P, c_int, P, P], c_int),
    "jlm_complete_frames_masked": ([POINTER(DecodeModel), POINTER(CompletePlan), P, c_int, c_int, P, P, P], c_int),
    "jlm_rank_rows": ([P, c_int, c_int, c_int, P, P, P, c_int, P, P, P, c_int, P, P, P], c_int),
    "jlm_rank_frames": ([POINTER(DecodeModel), POINTER(RankPlan), P, P], c_int),
    "jlm_cache_rows": ([P, P, c_int, c_int, c_int, c_int, c_float, c_int, c_int, P, P, c_int, POINTER(c_float), c_int, P, P, P], c_int),
    "jlm_score_cache_frames": ([POINTER(DecodeModel), POINTER(ScorePlan), POINTER(CachePlan), P, P], c_int),
    "jlm_memory_keys_per_split": ([c_int], c_int),
    "jlm_memory_workspace_bytes": ([c_int, c_int, c_int, c_int], c_size_t),
    "jlm_memory_rows": ([P, P, c_int, c_int, c_int, c_float, P, P, c_int, c_int, P, POINTER(c_float), c_int, P, P, c_size_t, P, P], c_int),
    "jlm_score_memory_frames": ([POINTER(DecodeModel), POINTER(ScorePlan), POINTER(MemoryPlan), P, P], c_int),
    "jlm_memory_topk_workspace_bytes": ([c_int, c_int, c_int], c_size_t),
    "jlm_memory_topk_chunk_keys": ([c_int, c_int, c_int, c_size_t], c_int),
    "jlm_memory_topk": ([P, P, c_int, c_int, c_int, c_float, P, c_int, P, c_float, c_int, P, c_int, P, P, c_int, P, c_size_t, P, P], c_int),
    "jlm_rank_memory_frames": ([POINTER(DecodeModel), POINTER(RankPlan), POINTER(MemoryMixPlan), P, P], c_int),
    "jlm_predict_memory_rows": ([POINTER(DecodeModel), POINTER(PredictMemoryPlan), P], c_int),
    "jlm_cache_query": ([P, c_int, c_int, c_int, c_int, c_float, P, c_int, P, c_int, P, c_int, c_float, P, c_int, P, P], c_int),
    "jlm_cache_mix_rows": ([P, c_int, c_int, c_int, P, c_int, P, c_int, c_int, c_int, P, c_int, P, c_int, c_float, P, P, P], c_int),
    "jlm_rank_cache_frames": ([POINTER(DecodeModel), POINTER(RankPlan), POINTER(CacheMixPlan), P, P], c_int),
    "jlm_predict_cache_rows": ([POINTER(DecodeModel), POINTER(PredictCachePlan), P], c_int),
    "jlm_prime_frames": ([POINTER(DecodeModel), POINTER(PrimePlan), P], c_int),
    "jlm_seed_context": ([P, P, c_int, P, P, c_int, P, c_int, c_int, c_longlong, P, P, P, P, P], c_int),
    "jlm_cache_cell_query": ([P, c_int, c_int, c_float, P, P, P, c_int, c_int, c_int, P, P, c_int, c_int, P, c_int, c_float, P, c_int, P, P],
                             c_int),
    "jlm_cache_cell_patch": ([P, c_int, P, P, c_int, c_int, P, c_int, c_float, P, P, c_int, c_int, c_int, P, P, P, c_int, P, P, P, c_int, c_int,
                              P, P, P, P], c_int),
    "jlm_ngram_cell_patch": ([P, P, c_int, c_int, c_int, c_float, P, P, P, c_int, c_int, c_int, P, P, P, P, P, P, P, c_int, P, P, P, c_int, c_int,
                              P, P, P, P], c_int),
    "jlm_memory_gather_rows": ([P, c_int, c_longlong, P, P, c_int, P, P], c_int),
    "jlm_memory_cell_patch": ([P, c_int, P, c_int, c_int, c_int, c_float, P, P, c_int, c_int, c_int, P, P, P, c_int, P, P, P, c_int, c_int,
                               P, P, P, P], c_int),
    "jlm_ngram_mix_refuse": ([P, c_int, c_int, POINTER(NgramRows), P, c_int, P, c_float, c_int, P], c_int),
    "jlm_ngram_mix_rows": ([P, c_int, c_int, c_int, POINTER(NgramRows), P, c_int, P, c_float, c_int, P, P], c_int),
    "jlm_ngram_hist_advance": ([P, c_int, P, P, c_int, P, P], c_int),
    "jlm_rank_ngram_frames": ([POINTER(DecodeModel), POINTER(RankPlan), POINTER(NgramMixPlan), P, P], c_int),
    "jlm_complete_frames_ngram": ([POINTER(DecodeModel), POINTER(CompletePlan), POINTER(CompleteNgramPlan), P, c_int, c_int, P, P, P], c_int),
    "jlm_prime_cache_frames": ([POINTER(DecodeModel), POINTER(PrimePlan), P, P, P, c_int, P], c_int),
    "jlm_tail_predict": ([POINTER(Segment), c_int, P, P, c_int, c_int, c_int, c_int, P, P, P, P, P, c_int, P, c_int, P, P, P, P, c_int, c_int,
                          P, P, P, P, P, c_int, P], c_int),
    "jlm_alt_head_refuse": ([POINTER(Segment), c_int, P, c_int, c_int, c_int, POINTER(AltPlan), POINTER(ScorePlan)], c_int),
    "jlm_alt_head": ([POINTER(Segment), c_int, P, c_int, c_int, c_int, POINTER(AltPlan), POINTER(ScorePlan), P], c_int),
    "jlm_alt_frames": ([POINTER(DecodeModel), POINTER(AltPlan), POINTER(ScorePlan), P, P], c_int),
    "jlm_vocab_lse_mixed_form": ([POINTER(Segment), POINTER(c_float), POINTER(c_float), c_int, c_int, c_int], c_int),
    "jlm_vocab_lse_split_form": ([], c_int),
    "jlm_gemm_nt_split_form": ([c_int, c_int], c_int),
    "jlm_wordlist_lse_form": ([POINTER(Segment), c_int, POINTER(Segment), c_int, c_int, c_int, c_int], c_int),
    "jlm_wordlist_merge_form": ([POINTER(Segment), c_int, POINTER(Segment), c_int, c_int, c_int], c_int),
    "jlm_beam_step_form": ([c_int, c_int, c_int, c_int], c_int),
    "jlm_backtrace_form": ([c_int, c_int], c_int),
    "jlm_kmeans1d": ([P, c_longlong, c_int, c_uint64, c_int, c_double, P, P, P, c_int, POINTER(c_int), POINTER(c_float), P], c_int),
    "jlm_train_gemm": ([P, c_longlong, c_longlong, P, c_longlong, c_longlong, P, c_int, c_int, c_int, c_int, c_int, P, P], c_int),
    "jlm_train_embed_rows": ([P, c_int, c_int, P, c_int, c_int, P, c_uint64, c_uint, c_float, P], c_int),
    "jlm_train_cell_fwd": ([P, P, P, P, P, c_int, c_int, c_longlong, c_uint64, c_uint, c_float, P], c_int),
    "jlm_train_cell_bwd": ([P, P, P, P, P, P, P, c_int, c_int, c_longlong, c_uint64, c_uint, c_float, P], c_int),
    "jlm_train_lse_update": ([P, c_int, c_int, c_int, P, P, c_int, P], c_int),
    "jlm_train_dy": ([P, c_int, c_int, c_int, c_int, P, P, P, P, c_float, c_float, P], c_int),
    "jlm_train_colsum": ([P, c_int, c_int, c_int, P, c_int, P], c_int),
    "jlm_train_ce": ([P, P, P, c_int, c_float, P, P, P], c_int),
    "jlm_distill_lse_update": ([P, c_int, P, c_int, c_int, c_int, c_float, P, c_int, P], c_int),
    "jlm_distill_dy": ([P, c_int, P, c_int, c_int, c_int, c_int, P, P, P, P, c_float, c_float, c_float, c_float, c_float, c_int, P], c_int),
    "jlm_distill_kl": ([P, c_int, P, P, P], c_int),
    "jlm_train_scatter_rows": ([P, c_int, c_int, c_int, c_int, P, P, c_int, P, c_int, c_int, c_int, c_uint64, c_uint, c_float, P], c_int),
    "jlm_train_adam": ([P, P, P, P, c_longlong, c_float, P, P], c_int),
    "jlm_train_gemm_splitk": ([P, c_longlong, c_longlong, P, c_longlong, c_longlong, P, c_int, c_int, c_int, c_int, c_int, P, c_int, P,
                               c_longlong, P], c_int),
    "jlm_dyneval_sqacc": ([P, P, c_longlong, P, P], c_int),
    "jlm_dyneval_rms": ([P, c_longlong, c_float, P, c_longlong, P, P, P], c_int),
    "jlm_dyneval_update": ([P, P, P, P, c_longlong, c_double, c_double, c_double, P, P], c_int),
    "jlm_train_expand_codes": ([P, c_int, P, P, c_longlong, P], c_int),
    "jlm_train_codebook_grad": ([P, c_longlong, P, c_longlong, P, c_int, c_int, P, P, P], c_int),
}
EXPORTS = sorted(_SIGS)

_lib = None


class JlmHipError(RuntimeError):
    pass


def lib():
    """The loaded shared library (argtypes set).  Raises when it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise JlmHipError(
                "libjlm_hip.so is not built (%s).  Build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'`; there is no CPU fallback." % LIB_PATH)
        # torch first: its bundled HIP runtime must be the one in the process before this
        # library (linked against libamdhip64) is mapped, or the two runtimes disagree
        # about the device (hipErrorNoDevice on the first launch).
        import torch  # noqa: F401
        l = ctypes.CDLL(LIB_PATH)
        for name, (args, res) in _SIGS.items():
            fn = getattr(l, name)
            fn.argtypes = args
            fn.restype = res
        if l.jlm_abi_version() != 12:
            raise JlmHipError("libjlm_hip.so ABI version mismatch")
        _lib = l
    return _lib


def require_gpu():
    import torch
    if not torch.cuda.is_available():
        raise JlmHipError("no GPU visible: jlm_amd runs only on MI355X (gfx950); there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def check(rc, what):
    if rc != 0:
        raise JlmHipError("%s failed with code %d" % (what, rc))
