"""The numpy double of ``jlm_cache_query`` / ``jlm_cache_mix_rows`` / ``jlm_rank_cache_frames`` / ``jlm_predict_cache_rows`` and of
``torch.ops.jlm.rank_cache_frames`` / ``predict_cache_rows`` for the CPU-only suite: tests/fake_rank.py's and tests/fake_cache.py's
doubles with the entry points more (those files stay as they are).  TEST INFRASTRUCTURE ONLY; it restates the contract written in
include/jlm_hip.h, not the HIP code: the sums are numpy's, in float64, rounded to float32 where the header says a value is one.
"""
import ctypes

import numpy as np

from jlm_amd.complete import topk_masked_reference, topk_reference
from tests import fake_cache, fake_hip, fake_rank
from tests.fake_cache import decode_rows
from tests.fake_hip import _n, _p, view

MAX_N = 4096
TOPK_MAX = 64


def _refuse_rings(cap, n_rows, n_rows_max, pos, first, n_dev, N, ld_s, flags):
    if n_rows < 0 or n_rows_max < 0 or n_rows_max > n_rows or N < 1 or N > MAX_N or cap < N or pos < 0 or ld_s < N:
        return -1
    if pos + cap > 0x7fffffff:
        return -1
    if n_rows_max == 0:
        return 0
    if n_rows_max > 65535 or not _p(first) or any(_p(x) % 4 for x in (first, n_dev, flags)):
        return -1
    return 0


def refuse_query(hist, cap, n_rows, H, split, h_scale, q_rows, n_rows_max, n_dev, pos, first, N, theta, s, ld_s, flags):
    rc = _refuse_rings(cap, n_rows, n_rows_max, pos, first, n_dev, N, ld_s, flags)
    if rc:
        return rc
    if H <= 0 or H % 32 or not (np.isfinite(theta) and theta >= 0) or (split and not (np.isfinite(h_scale) and h_scale > 0)):
        return -1
    if n_rows_max == 0:
        return 0
    if not all(_p(x) for x in (hist, q_rows, s)) or _p(hist) % 16 or _p(q_rows) % 16 or _p(s) % 4:
        return -1
    return 0


def refuse_mix(y, ld_y, n_cols, s, ld_s, words, cap, n_rows, n_rows_max, n_dev, pos, first, N, lam, lpc_ent, flags):
    rc = _refuse_rings(cap, n_rows, n_rows_max, pos, first, n_dev, N, ld_s, flags)
    if rc:
        return rc
    if not 0 <= lam < 1 or n_cols < 1 or ld_y % 4 or ld_y < (n_cols + 3) // 4 * 4:
        return -1
    if n_rows_max == 0:
        return 0
    if not all(_p(x) for x in (y, s, words)) or _p(y) % 16 or any(_p(x) % 4 for x in (s, words, lpc_ent)):
        return -1
    return 0


class MixLib(fake_rank.RankLib, fake_cache.CacheLib):
    def __init__(self):
        self.launches = []                # the entry points called, in order (a refused call launches nothing)

    def jlm_cache_query(self, hist, cap, n_rows, H, split, h_scale, q_rows, n_rows_max, n_dev, pos, first, N, theta, s, ld_s, flags, stream):
        rc = refuse_query(hist, cap, n_rows, H, split, h_scale, q_rows, n_rows_max, n_dev, pos, first, N, theta, s, ld_s, flags)
        if rc or n_rows_max == 0:
            return rc
        self.launches.append("cache_query")
        n = _n(n_rows_max, n_dev)
        if n <= 0:
            return 0
        hv = decode_rows(view(hist, cap * n_rows * H, np.float32).reshape(cap, n_rows, H), split, h_scale)
        qv = decode_rows(view(q_rows, n * H, np.float32).reshape(n, H), split, h_scale)
        fv = view(first, n_rows, np.int32)
        out = view(s, n * ld_s, np.float32).reshape(n, ld_s)
        bad = False
        for r in range(n):
            idx = np.arange(max(pos - N, int(fv[r]), 0), pos)
            if not len(idx):
                continue
            with np.errstate(invalid="ignore", over="ignore"):
                out[r, :len(idx)] = (float(np.float32(theta)) * (hv[idx % cap, r] @ qv[r])).astype(np.float32)
            bad |= not np.all(np.isfinite(out[r, :len(idx)]))
        if bad and _p(flags):
            view(flags, 1, np.int32)[0] |= 1
        return 0

    def jlm_cache_mix_rows(self, y, ld_y, n_cols, self_norm, s, ld_s, words, cap, n_rows, n_rows_max, n_dev, pos, first, N, lam, lpc_ent,
                           flags, stream):
        rc = refuse_mix(y, ld_y, n_cols, s, ld_s, words, cap, n_rows, n_rows_max, n_dev, pos, first, N, lam, lpc_ent, flags)
        if rc or n_rows_max == 0 or lam == 0:
            return rc
        self.launches.append("cache_mix_rows")
        n = _n(n_rows_max, n_dev)
        if n <= 0:
            return 0
        yv = view(y, n * ld_y, np.float32).reshape(n, ld_y)
        sv = view(s, n * ld_s, np.float32).reshape(n, ld_s)
        wv = view(words, cap * n_rows, np.int32).reshape(cap, n_rows)
        fv = view(first, n_rows, np.int32)
        ent = view(lpc_ent, n * ld_s, np.float32).reshape(n, ld_s) if _p(lpc_ent) else None
        lam32 = float(np.float32(lam))
        log_rho = float(np.float32(np.log(lam32) - np.log1p(-lam32)))
        fl = 0
        for r in range(n):
            idx = np.arange(max(pos - N, int(fv[r]), 0), pos)
            k = len(idx)
            if not k:
                continue
            sc = sv[r, :k].astype(np.float64)
            ww = wv[idx % cap, r]
            if np.any((ww < 0) | (ww >= n_cols)):
                fl |= 4
            if not np.all(np.isfinite(sc)):
                fl |= 1
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
            e = np.exp(sc - sc.max())
            logZ = np.log(e.sum())
            seen = set()
            for j in range(k):
                w = int(ww[j])
                if w in seen:
                    if ent is not None:
                        ent[r, j] = -np.inf
                    continue
                seen.add(w)
                with np.errstate(divide="ignore"):
                    lpc = np.float32(np.log(e[ww == w].sum()) - logZ)
                if ent is not None:
                    ent[r, j] = lpc
                if not 0 <= w < n_cols or np.isnan(row[w]) or np.isneginf(lpc):
                    continue
                yv[r, w] = np.float32(np.logaddexp(row[w], float(np.float32(L)) + log_rho + float(lpc)))
        if fl and _p(flags):
            view(flags, 1, np.int32)[0] |= fl
        return 0

    def jlm_topk_rows(self, y, ld_y, n_cols, n_rows, k, self_norm, ids, nll, ld_out, flags, stream, sets=None):
        if n_cols < 1 or ld_y % 4 or ld_y < (n_cols + 3) // 4 * 4 or not _p(y) or _p(y) % 16:
            return -1
        if not 1 <= k <= min(TOPK_MAX, n_cols) or ld_out < k or not _p(ids) or not _p(nll):
            return -1
        if n_rows <= 0:
            return 0
        self.launches.append("topk_rows")
        yv = view(y, n_rows * ld_y, np.float32).reshape(n_rows, ld_y)
        iv = view(ids, n_rows * ld_out, np.int32).reshape(n_rows, ld_out)
        nv = view(nll, n_rows * ld_out, np.float64).reshape(n_rows, ld_out)
        for r in range(n_rows):
            row = yv[r, :n_cols]
            if sets is not None and sets[r] is not None:
                i, v = topk_masked_reference(row, k, sets[r], bool(self_norm))
            else:
                i, v = topk_reference(row, k, bool(self_norm))
            ok = np.isfinite(row.astype(np.float64).max()) and (self_norm or np.isfinite(v[np.isfinite(v)]).all())
            if not ok:
                iv[r, :k], nv[r, :k] = -1, np.nan
                if _p(flags):
                    view(flags, 1, np.int32)[0] |= 1
                continue
            iv[r, :k], nv[r, :k] = i, v
        return 0

    def _step(self, m, h_in, c_in, h_out, c_out, T_rows, rows, prev, word, bound, ndev, logits, ld_logits, stream, lstm=True):
        """the LSTM step (``lstm``), the T projection and the logit GEMMs of ``bound`` rows, as RankLib.jlm_rank_frames makes them"""
        at = lambda base, n: _p(base) + 4 * n
        t_is_state = bool(m.untied) and not m.split_lstm
        T = h_out if t_is_state else T_rows
        if lstm:
            if m.split_lstm:
                rc = self.jlm_lstm_step_xg(h_in, c_in, m.H, h_out, c_out, rows, prev, word, m.wt8, m.xgate8, m.H, m.gate_descale, m.h_scale,
                                           T_rows if m.untied else None, bound, ndev, stream)
            else:
                rc = self.jlm_lstm_step(h_in, c_in, m.H, h_out, c_out, rows, prev, word, m.emb, m.ld_emb, m.wt, m.gate_bias, m.kpad, m.H, m.E,
                                        bound, ndev, stream)
            if rc:
                return rc
        if not m.untied:
            if m.split_lstm:
                rc = self.jlm_gemm_nt_split(h_out, m.H, rows, m.pmt_split, m.H, None, T, m.ldt, rows, None, m.t_descale, bound, m.n_t, m.H,
                                            ndev, stream)
            else:
                rc = self.jlm_gemm_nt(h_out, m.H, rows, m.pmt, m.H, None, T, m.ldt, rows, None, bound, m.n_t, m.H, ndev, stream)
            if rc:
                return rc
        for i in range(m.n_segs):
            sg = m.segs[i]
            rc = self.jlm_gemm_nt(at(T, sg.t_off), m.ldt, None, sg.B, sg.ldb, None, at(logits, sg.v_start), ld_logits, None,
                                  at(m.b2, sg.v_start), bound, sg.v_end - sg.v_start, sg.k, None, stream)
            if rc:
                return rc
        return 0

    def jlm_rank_cache_frames(self, m, p, cp, stream, events=None):
        R, S = p.n_rows, p.n_steps
        if R < 0 or S < 0 or cp.pos0 < 0 or cp.pos0 + S > 0x7fffffff:
            return -1
        split = 1 if m.split_lstm else 0
        V = m.segs[m.n_segs - 1].v_end
        last = cp.pos0 + max(S - 1, 0)
        rc = refuse_query(cp.hist, cp.cap, R, m.H, split, m.h_scale, p.h[0], R, p.n_live, last, cp.first, cp.N, cp.theta, cp.s, cp.ld_s, cp.flags)
        rc = rc or refuse_mix(p.logits, p.ld_logits, V, cp.s, cp.ld_s, cp.words, cp.cap, R, R, p.n_live, last, cp.first, cp.N, cp.lam, None,
                              cp.flags)
        if rc:
            return rc
        if not 0 <= cp.top_k <= min(TOPK_MAX, V) or (cp.top_k and not (_p(cp.top_ids) and _p(cp.top_nll) and p.n_live_host)):
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
        self.launches.append("rank_cache_frames")
        at = lambda base, n: _p(base) + 4 * n
        hist = view(cp.hist, cp.cap * R * m.H, np.float32).reshape(cp.cap, R, m.H)
        words = view(cp.words, cp.cap * R, np.int32).reshape(cp.cap, R)
        for t in range(S):
            bound = int(p.n_live_host[t]) if p.n_live_host else R
            if bound == 0:
                continue
            ndev = at(p.n_live, t)
            h_in, h_out, c_in, c_out = p.h[t & 1], p.h[(t + 1) & 1], p.c[t & 1], p.c[(t + 1) & 1]
            rc = self._step(m, h_in, c_in, h_out, c_out, p.T, p.rows, p.prev0 if t == 0 else p.rows, at(p.word, t * R), bound, ndev, p.logits,
                            p.ld_logits, stream)
            pos = cp.pos0 + t
            rc = rc or self.jlm_cache_query(cp.hist, cp.cap, R, m.H, split, m.h_scale, h_out, bound, ndev, pos, cp.first, cp.N, cp.theta, cp.s,
                                            cp.ld_s, cp.flags, stream)
            rc = rc or self.jlm_cache_mix_rows(p.logits, p.ld_logits, V, m.self_norm, cp.s, cp.ld_s, cp.words, cp.cap, R, bound, ndev, pos,
                                               cp.first, cp.N, cp.lam, None, cp.flags, stream)
            rc = rc or self.jlm_rank_rows(p.logits, p.ld_logits, V, bound, ndev, at(p.target, t * R), p.ids, p.n_ids, p.lv_off, p.lv_lo,
                                          p.lv_hi, p.n_levels, at(p.rank, t * R * (p.n_levels + 1)), p.flags, stream)
            if not rc and cp.top_k:
                rc = self.jlm_topk_rows(p.logits, p.ld_logits, V, bound, cp.top_k, m.self_norm, at(cp.top_ids, t * R * cp.top_k),
                                        _p(cp.top_nll) + 8 * t * R * cp.top_k, cp.top_k, p.flags, stream)
            if rc:
                return rc
            slot = pos % cp.cap
            hist[slot, :bound] = view(h_out, R * m.H, np.float32).reshape(R, m.H)[:bound]
            words[slot, :bound] = view(at(p.target, t * R), R, np.int32)[:bound]
        return 0

    def jlm_predict_cache_rows(self, m, p, stream, sets=None):
        R = p.n_rows
        if R < 0 or not all(_p(x) for x in (p.rows, p.logits, p.ids, p.nll)):
            return -1
        if m.untied and m.split_lstm:
            return -2
        split = 1 if m.split_lstm else 0
        V = m.segs[m.n_segs - 1].v_end
        rc = refuse_query(p.hist, p.cap, R, m.H, split, m.h_scale, p.h, R, None, p.pos, p.first, p.N, p.theta, p.s, p.ld_s, p.cache_flags)
        rc = rc or refuse_mix(p.logits, p.ld_logits, V, p.s, p.ld_s, p.words, p.cap, R, R, None, p.pos, p.first, p.N, p.lam, None,
                              p.cache_flags)
        if rc or not 1 <= p.k <= min(TOPK_MAX, V):
            return rc or -1
        if R == 0:
            return 0
        if not _p(p.T) and not (bool(m.untied) and not m.split_lstm):
            return -1
        self.launches.append("predict_cache_rows")
        rc = self._step(m, None, None, p.h, None, p.T, p.rows, None, None, R, None, p.logits, p.ld_logits, stream, lstm=False)
        rc = rc or self.jlm_cache_query(p.hist, p.cap, R, m.H, split, m.h_scale, p.h, R, None, p.pos, p.first, p.N, p.theta, p.s, p.ld_s,
                                        p.cache_flags, stream)
        rc = rc or self.jlm_cache_mix_rows(p.logits, p.ld_logits, V, m.self_norm, p.s, p.ld_s, p.words, p.cap, R, R, None, p.pos, p.first,
                                           p.N, p.lam, None, p.cache_flags, stream)
        return rc or self.jlm_topk_rows(p.logits, p.ld_logits, V, R, p.k, m.self_norm, p.ids, p.nll, p.k, p.flags, stream, sets=sets)


class MixOps(fake_rank.RankOps, fake_cache.CacheOps):
    def __init__(self, lib=None):
        fake_hip.FakeOps.__init__(self, lib or MixLib())

    def rank_cache_frames(self, model, h0, c0, h1, c1, T, logits, ld_logits, rows, prev0, word, target, n_live, n_live_host, ids, lv_off,
                          lv_lo, lv_hi, n_levels, rank, flags, n_rows, n_steps, timed, hist, words, cap, pos0, first, N, theta, lam, s,
                          ld_s, top_k, top_ids, top_nll, cache_flags):
        import torch
        from jlm_amd import _lib
        o, m = self._o, model.m
        R, S = int(n_rows), int(n_steps)
        assert len(n_live_host) == S and all(0 <= x <= R for x in n_live_host)
        assert word.numel() >= S * R and target.numel() >= S * R and rank.numel() >= S * R * (n_levels + 1) and logits.numel() >= R * ld_logits
        assert hist.numel() >= cap * R * m.H and words.numel() >= cap * R and first.numel() >= R and s.numel() >= R * ld_s
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
        cp = _lib.CacheMixPlan()
        cp.hist, cp.words, cp.cap, cp.pos0, cp.first, cp.N = o(hist), o(words), int(cap), int(pos0), o(first), int(N)
        cp.theta, cp.lam, cp.s, cp.ld_s, cp.top_k = float(theta), float(lam), o(s), int(ld_s), int(top_k)
        cp.top_ids, cp.top_nll, cp.flags = o(top_ids), o(top_nll), o(cache_flags)
        self._chk(self.lib.jlm_rank_cache_frames(m, p, cp, 0, None), "jlm_rank_cache_frames")
        return torch.full((S, 6), 1e-3, dtype=torch.float64) if timed and R > 0 else torch.empty(0, dtype=torch.float64)

    def predict_cache_rows(self, model, h, T, logits, ld_logits, rows, hist, words, cap, pos, first, N, theta, lam, s, ld_s, k, mask, ld_mask,
                           n_sets, row_set, ids, nll, flags, cache_flags, n_rows):
        from jlm_amd import _lib
        o, m = self._o, model.m
        R = int(n_rows)
        if m.untied and m.split_lstm:
            raise RuntimeError("jlm.predict_cache_rows: an untied split-row model has no one-step form")
        assert h.numel() >= R * m.H and logits.numel() >= R * ld_logits and ids.numel() >= R * k and nll.numel() >= R * k
        assert hist.numel() >= cap * R * m.H and words.numel() >= cap * R and first.numel() >= R and s.numel() >= R * ld_s
        sets = None
        if mask is not None:
            assert len(row_set) == R and all(-1 <= x < n_sets for x in row_set)
            bits = mask.numpy().view(np.uint32).reshape(-1)[:n_sets * ld_mask].reshape(n_sets, ld_mask)
            V = m.segs[m.n_segs - 1].v_end
            member = lambda q: np.flatnonzero((bits[q][np.arange(V) >> 5] >> (np.arange(V) & 31).astype(np.uint32)) & 1)
            sets = [None if q < 0 else member(q) for q in row_set]
        p = _lib.PredictCachePlan()
        p.n_rows, p.h, p.T, p.logits, p.ld_logits, p.rows = R, o(h), o(T), o(logits), int(ld_logits), o(rows)
        p.hist, p.words, p.cap, p.pos, p.first, p.N = o(hist), o(words), int(cap), int(pos), o(first), int(N)
        p.theta, p.lam, p.s, p.ld_s, p.k = float(theta), float(lam), o(s), int(ld_s), int(k)
        p.ids, p.nll, p.flags, p.cache_flags = o(ids), o(nll), o(flags), o(cache_flags)
        self._chk(self.lib.jlm_predict_cache_rows(m, p, 0, sets=sets), "jlm_predict_cache_rows")


def install(monkeypatch):
    """fake_hip.install with the doubles above"""
    import torch
    from jlm_amd import _lib, ops

    fake = MixLib()
    monkeypatch.setattr(_lib, "lib", lambda: fake)
    monkeypatch.setattr(_lib, "require_gpu", lambda: torch.device("cpu"))
    monkeypatch.setattr(ops, "_backend", MixOps(fake))
    return fake
