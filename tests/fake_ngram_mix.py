"""The numpy double of ``jlm_ngram_mix_rows`` / ``jlm_ngram_hist_advance`` / ``jlm_rank_ngram_frames`` / ``jlm_complete_frames_ngram``
(and of the plain ``jlm_complete_frames`` / ``jlm_complete_frames_masked`` they extend) and of ``torch.ops.jlm.rank_ngram_frames`` /
``complete_frames`` / ``complete_frames_masked`` / ``complete_frames_ngram`` for the CPU-only suite: tests/fake_cache_mix.py's doubles
with the entry points more (that file stays as it is).  TEST INFRASTRUCTURE ONLY; it restates the contract written in
include/jlm_hip.h, not the HIP code: q is summed in the float32 order the header gives, the mixture is numpy's in float64, rounded to
float32 once.
"""
import ctypes

import numpy as np

from jlm_amd.complete import merge_reference
from tests import fake_cache_mix, fake_hip, fake_rank
from tests.fake_hip import _n, _p, view

MAX_V = 393216
GOLDEN = 0x9E3779B97F4A7C15


def _table(t):
    return t.contents if hasattr(t, "contents") else getattr(t, "_obj", t)


def refuse_mix(y, ld_y, n_cols, table, hist, n_rows, n_dev, lam, order, flags):
    if not table:
        return -1
    t = _table(table)
    if not 1 <= order <= 3 or not 0 < lam < 1:
        return -1
    if not 1 <= n_cols <= MAX_V or ld_y % 4 or ld_y < (n_cols + 3) // 4 * 4:
        return -1
    if n_rows < 0 or t.n_bi < 0 or t.n_tri < 0 or t.n_ctx < 0 or not 6 <= t.log2cap <= 31 or not 0 <= t.max_probe < (1 << t.log2cap):
        return -1
    ptrs = [t.uni_lp, t.uni_bow, t.bi_off, t.bi_w, t.bi_lp, t.tri_off, t.tri_w, t.tri_lp, t.tri_bow, t.ctx_vals]
    if not all(_p(x) for x in ptrs) or not _p(t.ctx_keys):
        return -1
    if any(_p(x) % 4 for x in ptrs + [hist, n_dev, flags]) or _p(t.ctx_keys) % 8:
        return -1
    if n_rows == 0:
        return 0
    if not _p(y) or not _p(hist) or _p(y) % 16:
        return -1
    return 0


def context_index(t, u, v):
    """the probe of the context map as the header states it: the key, an empty slot, or max_probe + 1 slots"""
    cap = 1 << t.log2cap
    keys = np.frombuffer((ctypes.c_uint64 * cap).from_address(_p(t.ctx_keys)), dtype=np.uint64)
    vals = view(t.ctx_vals, cap, np.int32)
    key = (v + 1) | ((u + 1) << 21)
    slot = ((key * GOLDEN) & ((1 << 64) - 1)) >> (64 - t.log2cap)
    for i in range(t.max_probe + 1):
        k = int(keys[slot])
        if k == key:
            return int(vals[slot])
        if k == 0:
            return -1
        slot = (slot + 1) & (cap - 1)
    return -1


def walk(t, V, u, v, order):
    """q(. | (u, v)) over V words from the successor arrays, in the float32 order of the header: a trigram successor's lp; bow(u v) +
    lp of a bigram successor no trigram covered; (bow(u v) + bow(v)) + lp of every remaining word with a unigram; -inf elsewhere.
    Indices that point outside the arrays are skipped.  -> float32 [V]"""
    f32 = np.float32
    if order < 2:
        v = -1
    if order < 3 or v < 0:
        u = -1
    q = np.full(V, -np.inf, dtype=f32)
    done = np.zeros(V, dtype=bool)
    w1 = w2 = f32(0.0)

    def take(ws, lps, add):
        for w, lp in zip(ws.tolist(), lps):
            if 0 <= w < V and not done[w]:
                done[w] = True
                q[w] = f32(add + lp)

    if v >= 0:
        w1 = view(t.uni_bow, V, f32)[v]
        b0, b1 = (int(x) for x in view(t.bi_off, V + 1, np.int32)[v:v + 2])
        c = context_index(t, u, v) if u >= 0 else -1
        if 0 <= c < t.n_ctx:
            t0, t1 = (int(x) for x in view(t.tri_off, t.n_ctx + 1, np.int32)[c:c + 2])
            w2 = view(t.tri_bow, t.n_ctx, f32)[c]
            if 0 <= t0 <= t1 <= t.n_tri and t1 > t0:
                take(view(t.tri_w, t.n_tri, np.int32)[t0:t1], view(t.tri_lp, t.n_tri, f32)[t0:t1], f32(0.0))
        if 0 <= b0 <= b1 <= t.n_bi and b1 > b0:
            take(view(t.bi_w, t.n_bi, np.int32)[b0:b1], view(t.bi_lp, t.n_bi, f32)[b0:b1], w2)
    back = f32(w2 + w1)
    uni = view(t.uni_lp, V, f32)
    rest = ~done & np.isfinite(uni)
    q[rest] = (back + uni[rest]).astype(f32)
    return q


class NgramMixLib(fake_cache_mix.MixLib):
    jlm_ngram_mix_refuse = staticmethod(refuse_mix)

    def jlm_ngram_mix_rows(self, y, ld_y, n_cols, self_norm, table, hist, n_rows, n_dev, lam, order, flags, stream):
        rc = refuse_mix(y, ld_y, n_cols, table, hist, n_rows, n_dev, lam, order, flags)
        if rc or n_rows == 0:
            return rc
        self.launches.append("ngram_mix_rows")
        n = _n(n_rows, n_dev)
        if n <= 0:
            return 0
        t = _table(table)
        yv = view(y, n * ld_y, np.float32).reshape(n, ld_y)
        hv = view(hist, 2 * n, np.int32).reshape(n, 2)
        lam32 = float(np.float32(lam))
        log_rho = float(np.float32(np.log(lam32) - np.log1p(-lam32)))
        fl = 0
        for r in range(n):
            u, v = int(hv[r, 0]), int(hv[r, 1])
            if not (-1 <= u < n_cols and -1 <= v < n_cols):
                fl |= 4
                continue
            row = yv[r, :n_cols].astype(np.float64)
            L = 0.0
            if not self_norm:
                with np.errstate(invalid="ignore", over="ignore"):
                    top = row.max()
                    L = top + np.log(np.exp(row - top).sum())
                if not np.isfinite(L):
                    fl |= 2
                    continue
            q = walk(t, n_cols, u, v, order).astype(np.float64)
            at = np.isfinite(q) & ~np.isnan(row)
            yv[r, :n_cols][at] = np.logaddexp(row[at], float(np.float32(L)) + log_rho + q[at]).astype(np.float32)
        if fl and _p(flags):
            view(flags, 1, np.int32)[0] |= fl
        return 0

    def jlm_ngram_hist_advance(self, hist_in, n_in, prev_row, word, n, hist_out, stream):
        if n < 0 or n_in < 0:
            return -1
        if n == 0:
            return 0
        if not all(_p(x) for x in (hist_in, prev_row, word, hist_out)) or _p(hist_in) == _p(hist_out):
            return -1
        if _p(hist_in) % 8 or _p(hist_out) % 8 or _p(prev_row) % 4 or _p(word) % 4:
            return -1
        self.launches.append("ngram_hist_advance")
        hin = view(hist_in, 2 * max(n_in, 1), np.int32).reshape(-1, 2)
        pv, wv = view(prev_row, n, np.int32), view(word, n, np.int32)
        out = view(hist_out, 2 * n, np.int32).reshape(n, 2)
        ok = (pv >= 0) & (pv < n_in)
        out[:, 0] = np.where(ok, hin[np.clip(pv, 0, max(n_in - 1, 0)), 1], -1)
        out[:, 1] = wv
        return 0

    def jlm_rank_ngram_frames(self, m, p, np_, stream, events=None):
        R, S = p.n_rows, p.n_steps
        if R < 0 or S < 0:
            return -1
        V = m.segs[m.n_segs - 1].v_end
        rc = refuse_mix(p.logits, p.ld_logits, V, np_.table, np_.hist, R, p.n_live, np_.lam, np_.order, np_.flags)
        if rc:
            return rc
        if not 0 <= np_.top_k <= min(fake_cache_mix.TOPK_MAX, V) or (np_.top_k and not (_p(np_.top_ids) and _p(np_.top_nll) and p.n_live_host)):
            return -1
        if p.n_live_host and any(not 0 <= p.n_live_host[t] <= R for t in range(S)):
            return -1
        if not all(_p(x) for x in (p.rows, p.prev0, p.word, p.target, p.n_live, p.logits, p.rank)) or not 0 <= p.n_levels <= fake_rank.MAX_LEVELS:
            return -1
        if R == 0 or S == 0:
            return 0
        if m.split_lstm and not m.wt8:
            return -2
        if not _p(p.T) and not (bool(m.untied) and not m.split_lstm):
            return -1
        self.launches.append("rank_ngram_frames")
        at = lambda base, n: _p(base) + 4 * n
        for t in range(S):
            bound = int(p.n_live_host[t]) if p.n_live_host else R
            if bound == 0:
                continue
            ndev = at(p.n_live, t)
            h_in, h_out, c_in, c_out = p.h[t & 1], p.h[(t + 1) & 1], p.c[t & 1], p.c[(t + 1) & 1]
            rc = self._step(m, h_in, c_in, h_out, c_out, p.T, p.rows, p.prev0 if t == 0 else p.rows, at(p.word, t * R), bound, ndev, p.logits,
                            p.ld_logits, stream)
            rc = rc or self.jlm_ngram_mix_rows(p.logits, p.ld_logits, V, m.self_norm, np_.table, at(np_.hist, 2 * t * R), bound, ndev,
                                               np_.lam, np_.order, np_.flags, stream)
            rc = rc or self.jlm_rank_rows(p.logits, p.ld_logits, V, bound, ndev, at(p.target, t * R), p.ids, p.n_ids, p.lv_off, p.lv_lo,
                                          p.lv_hi, p.n_levels, at(p.rank, t * R * (p.n_levels + 1)), p.flags, stream)
            if not rc and np_.top_k:
                rc = self.jlm_topk_rows(p.logits, p.ld_logits, V, bound, np_.top_k, m.self_norm, at(np_.top_ids, t * R * np_.top_k),
                                        _p(np_.top_nll) + 8 * t * R * np_.top_k, np_.top_k, p.flags, stream)
            if rc:
                return rc
        return 0

    # ------------------------------------------------------------------------------------------------ completion
    def jlm_beam_merge(self, cand_ids, cand_nll, beam, n_prompts, first, stop_id, word, prev, score, finished, bp_parent, bp_word, bp_nll,
                       stream):
        R, B = n_prompts * beam, beam
        n_src = n_prompts if first else R
        ci = view(cand_ids, n_src * B, np.int32).reshape(n_src, B)
        cn = view(cand_nll, n_src * B, np.float64).reshape(n_src, B)
        sc, fin = view(score, R, np.float64), view(finished, R, np.int32)
        out = merge_reference(ci, cn, sc.copy(), fin.copy(), B, n_prompts, bool(first), stop_id)
        self.launches.append("beam_merge")
        view(word, R, np.int32)[:] = out["word"]
        view(prev, R, np.int32)[:] = out["prev"]
        sc[:], fin[:] = out["score"], out["finished"]
        view(bp_parent, R, np.int32)[:] = out["bp_parent"]
        view(bp_word, R, np.int32)[:] = out["bp_word"]
        view(bp_nll, R, np.float64)[:] = out["bp_nll"]
        return 0

    def _complete(self, m, p, sets, np_, stream):
        """complete_frames of csrc/jlm_decode.hip restated: ``sets``: None or per prompt None / the ids frame 0 selects among; ``np_``:
        the n-gram plan or None"""
        NP, B, P, N = p.n_prompts, p.beam, p.n_prompt, p.n_words
        need = (p.rows, p.prev, p.prompt, p.n_live, p.n_live_host, p.logits, p.cand_ids, p.cand_nll, p.word, p.prev_row, p.score, p.finished,
                p.bp_parent, p.bp_word, p.bp_nll)
        if NP < 0 or not 1 <= B <= fake_cache_mix.TOPK_MAX or P < 1 or N < 0 or not all(_p(x) if not hasattr(x, "contents") else bool(x) for x in need):
            return -1
        if NP == 0 or N == 0:
            return 0
        if m.split_lstm and not m.wt8:
            return -2
        if not _p(p.T) and not (bool(m.untied) and not m.split_lstm):
            return -1
        V = m.segs[m.n_segs - 1].v_end
        if B > V or p.ld_logits % 4 or p.ld_logits < (V + 3) // 4 * 4 or p.n_live_host[P - 1] != NP:
            return -1
        R = NP * B
        at = lambda base, n: _p(base) + 4 * n
        for f in range(P + N - 1):
            h_in, h_out, c_in, c_out = p.h[f & 1], p.h[(f + 1) & 1], p.c[f & 1], p.c[(f + 1) & 1]
            in_prompt = f < P
            bound = int(p.n_live_host[f]) if in_prompt else R
            if bound < 0 or (in_prompt and bound > NP):
                return -1
            k = f - (P - 1)
            n_sel = NP if k == 0 else R
            rc = 0
            if bound > 0:
                prev = at(p.prev, f * NP) if in_prompt else p.prev_row
                word = at(p.prompt, f * NP) if in_prompt else p.word
                ndev = at(p.n_live, f) if in_prompt else None
                rc = self._lstm_only(m, h_in, c_in, h_out, c_out, p.T, p.rows, prev, word, bound, ndev, stream)
                if k >= 0:                                                  # a selecting frame: the T projection and the logit GEMMs
                    rc = rc or self._step(m, None, None, h_out, None, p.T, p.rows, None, None, n_sel, None, p.logits, p.ld_logits, stream,
                                          lstm=False)
            if rc:
                return rc
            if k < 0:
                continue
            if np_ is not None:
                rc = self.jlm_ngram_mix_rows(p.logits, p.ld_logits, V, m.self_norm, np_.table, np_.hist[k & 1], n_sel, None, np_.lam,
                                             np_.order, np_.flags, stream)
            rc = rc or self.jlm_topk_rows(p.logits, p.ld_logits, V, n_sel, B, m.self_norm, p.cand_ids, p.cand_nll, B, p.flags, stream,
                                          sets=sets if k == 0 else None)
            rc = rc or self.jlm_beam_merge(p.cand_ids, p.cand_nll, B, NP, k == 0, p.stop_id, p.word, p.prev_row, p.score, p.finished,
                                           at(p.bp_parent, k * R), at(p.bp_word, k * R), _p(p.bp_nll) + 8 * k * R, stream)
            if not rc and np_ is not None and k + 1 < N:
                rc = self.jlm_ngram_hist_advance(np_.hist[k & 1], n_sel, p.prev_row, p.word, R, np_.hist[(k + 1) & 1], stream)
            if rc:
                return rc
        return 0

    def _lstm_only(self, m, h_in, c_in, h_out, c_out, T_rows, rows, prev, word, bound, ndev, stream):
        if m.split_lstm:
            return self.jlm_lstm_step_xg(h_in, c_in, m.H, h_out, c_out, rows, prev, word, m.wt8, m.xgate8, m.H, m.gate_descale, m.h_scale,
                                         T_rows if m.untied else None, bound, ndev, stream)
        return self.jlm_lstm_step(h_in, c_in, m.H, h_out, c_out, rows, prev, word, m.emb, m.ld_emb, m.wt, m.gate_bias, m.kpad, m.H, m.E,
                                  bound, ndev, stream)

    def jlm_complete_frames(self, m, p, stream, events=None):
        self.launches.append("complete_frames")
        return self._complete(m, p, None, None, stream)

    def jlm_complete_frames_masked(self, m, p, sets, stream, events=None):
        self.launches.append("complete_frames_masked")
        return self._complete(m, p, sets, None, stream)

    def jlm_complete_frames_ngram(self, m, p, np_, sets, stream, events=None):
        if p.n_prompts < 0 or p.beam < 1:
            return -1
        R, V = p.n_prompts * p.beam, m.segs[m.n_segs - 1].v_end
        rc = refuse_mix(p.logits, p.ld_logits, V, np_.table, np_.hist[0], R, None, np_.lam, np_.order, np_.flags)
        if rc:
            return rc
        if R > 0 and p.n_words > 1 and (not _p(np_.hist[1]) or _p(np_.hist[1]) == _p(np_.hist[0]) or _p(np_.hist[0]) % 8 or _p(np_.hist[1]) % 8):
            return -1
        self.launches.append("complete_frames_ngram")
        return self._complete(m, p, sets, np_, stream)


def rows_struct(table, sizes):
    """the jlm_ngram_rows of an op's (table tensors, sizes)"""
    from jlm_amd import _lib
    from jlm_amd.ngram import SUCCESSOR_TENSORS
    t = _lib.NgramRows()
    assert len(table) == len(SUCCESSOR_TENSORS) and len(sizes) == 5
    for name, x in zip(SUCCESSOR_TENSORS, table):
        setattr(t, name, x.data_ptr())
    t.n_bi, t.n_tri, t.n_ctx, t.log2cap, t.max_probe = (int(x) for x in sizes)
    return t


class NgramMixOps(fake_cache_mix.MixOps):
    def __init__(self, lib=None):
        fake_hip.FakeOps.__init__(self, lib or NgramMixLib())

    def rank_ngram_frames(self, model, h0, c0, h1, c1, T, logits, ld_logits, rows, prev0, word, target, n_live, n_live_host, ids, lv_off,
                          lv_lo, lv_hi, n_levels, rank, flags, n_rows, n_steps, timed, table, sizes, order, lam, hist, top_k, top_ids,
                          top_nll, ngram_flags):
        import torch
        from jlm_amd import _lib
        o, m = self._o, model.m
        R, S = int(n_rows), int(n_steps)
        assert len(n_live_host) == S and all(0 <= x <= R for x in n_live_host)
        assert word.numel() >= S * R and target.numel() >= S * R and rank.numel() >= S * R * (n_levels + 1) and logits.numel() >= R * ld_logits
        assert hist.numel() >= 2 * S * R and hist.dtype == torch.int32
        assert top_k == 0 or (top_ids.numel() >= S * R * top_k and top_nll.numel() >= S * R * top_k)
        idp, n_ids, off, lo, hi = self._levels(ids, lv_off, lv_lo, lv_hi, m.segs[m.n_segs - 1].v_end, n_levels)
        p = _lib.RankPlan()
        p.n_rows, p.n_steps = R, S
        p.h[0], p.h[1], p.c[0], p.c[1], p.T = o(h0), o(h1), o(c0), o(c1), o(T)
        p.logits, p.ld_logits = o(logits), int(ld_logits)
        p.rows, p.prev0, p.word, p.target, p.n_live = o(rows), o(prev0), o(word), o(target), o(n_live)
        live = (ctypes.c_int * max(S, 1))(*[int(x) for x in n_live_host])
        p.n_live_host = ctypes.cast(live, ctypes.POINTER(ctypes.c_int))
        p.ids, p.n_ids, p.lv_off, p.lv_lo, p.lv_hi, p.n_levels = idp, n_ids, off, lo, hi, int(n_levels)
        p.rank, p.flags = o(rank), o(flags)
        t = rows_struct(table, sizes)
        np_ = _lib.NgramMixPlan()
        np_.table, np_.order, np_.lam, np_.hist, np_.top_k = ctypes.pointer(t), int(order), float(lam), o(hist), int(top_k)
        np_.top_ids, np_.top_nll, np_.flags = o(top_ids), o(top_nll), o(ngram_flags)
        self._chk(self.lib.jlm_rank_ngram_frames(m, p, np_, 0, None), "jlm_rank_ngram_frames")
        return torch.full((S, 5), 1e-3, dtype=torch.float64) if timed and R > 0 else torch.empty(0, dtype=torch.float64)

    def _complete_plan(self, model, h0, c0, h1, c1, T, logits, ld_logits, rows, prev, prompt, n_live, n_live_host, cand_ids, cand_nll, word,
                       prev_row, score, finished, stop_id, bp_parent, bp_word, bp_nll, flags, n_prompts, beam, n_prompt, n_words):
        from jlm_amd import _lib
        o = self._o
        p = _lib.CompletePlan()
        p.n_prompts, p.beam, p.n_prompt, p.n_words = int(n_prompts), int(beam), int(n_prompt), int(n_words)
        p.h[0], p.h[1], p.c[0], p.c[1], p.T = o(h0), o(h1), o(c0), o(c1), o(T)
        p.logits, p.ld_logits = o(logits), int(ld_logits)
        p.rows, p.prev, p.prompt, p.n_live = o(rows), o(prev), o(prompt), o(n_live)
        live = (ctypes.c_int * max(len(n_live_host), 1))(*[int(x) for x in n_live_host])
        p.n_live_host = ctypes.cast(live, ctypes.POINTER(ctypes.c_int))
        p._keep = live
        p.cand_ids, p.cand_nll, p.word, p.prev_row, p.score, p.finished = o(cand_ids), o(cand_nll), o(word), o(prev_row), o(score), o(finished)
        p.stop_id = int(stop_id)
        p.bp_parent, p.bp_word, p.bp_nll, p.flags = o(bp_parent), o(bp_word), o(bp_nll), o(flags)
        return p

    @staticmethod
    def _prompt_sets(mask, ld_mask, n_sets, prompt_set, V):
        if mask is None:
            return None
        bits = mask.numpy().view(np.uint32).reshape(-1)[:n_sets * ld_mask].reshape(n_sets, ld_mask)
        member = lambda q: np.flatnonzero((bits[q][np.arange(V) >> 5] >> (np.arange(V) & 31).astype(np.uint32)) & 1)
        return [None if q < 0 else member(q) for q in prompt_set]

    @staticmethod
    def _times(timed, n_prompts, n_prompt, n_words):
        import torch
        if timed and n_prompts > 0 and n_words > 0:
            return torch.full((n_prompt + n_words - 1, 5), 1e-3, dtype=torch.float64)
        return torch.empty(0, dtype=torch.float64)

    def complete_frames(self, model, *a):
        p = self._complete_plan(model, *a[:27])
        self._chk(self.lib.jlm_complete_frames(model.m, p, 0, None), "jlm_complete_frames")
        return self._times(a[27], p.n_prompts, p.n_prompt, p.n_words)

    def complete_frames_masked(self, model, *a):
        p = self._complete_plan(model, *a[:27])
        V = model.m.segs[model.m.n_segs - 1].v_end
        sets = self._prompt_sets(a[28], a[29], a[30], a[31], V)
        self._chk(self.lib.jlm_complete_frames_masked(model.m, p, sets, 0, None), "jlm_complete_frames_masked")
        return self._times(a[27], p.n_prompts, p.n_prompt, p.n_words)

    def complete_frames_ngram(self, model, *a):
        from jlm_amd import _lib
        p = self._complete_plan(model, *a[:27])
        V = model.m.segs[model.m.n_segs - 1].v_end
        sets = self._prompt_sets(a[28], a[29], a[30], a[31], V)
        table, sizes, order, lam, hist0, hist1, nflags = a[32:39]
        t = rows_struct(table, sizes)
        np_ = _lib.CompleteNgramPlan()
        np_.table, np_.order, np_.lam = ctypes.pointer(t), int(order), float(lam)
        np_.hist[0], np_.hist[1], np_.flags = self._o(hist0), self._o(hist1), self._o(nflags)
        self._chk(self.lib.jlm_complete_frames_ngram(model.m, p, np_, sets, 0, None), "jlm_complete_frames_ngram")
        return self._times(a[27], p.n_prompts, p.n_prompt, p.n_words)


def install(monkeypatch):
    """fake_hip.install with the doubles above"""
    import torch
    from jlm_amd import _lib, ops

    fake = NgramMixLib()
    monkeypatch.setattr(_lib, "lib", lambda: fake)
    monkeypatch.setattr(_lib, "require_gpu", lambda: torch.device("cpu"))
    monkeypatch.setattr(ops, "_backend", NgramMixOps(fake))
    return fake
