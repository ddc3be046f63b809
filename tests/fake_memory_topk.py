"""The numpy double of ``jlm_memory_topk`` / ``jlm_memory_topk_workspace_bytes`` / ``jlm_memory_topk_chunk_keys`` /
``jlm_rank_memory_frames`` / ``jlm_predict_memory_rows`` and of ``torch.ops.jlm.memory_topk`` / ``rank_memory_frames`` /
``predict_memory_rows`` for the CPU-only suite: tests/fake_memory.py's classes with tests/fake_cache_mix.py's patch, ranking loop and
lists, and the entry points more (those files stay as they are).  TEST INFRASTRUCTURE ONLY; it restates the contract written in
include/jlm_hip.h, not the HIP code: the order is the header's total order over float32 scores, by a stable sort.
"""
import ctypes

import numpy as np

from tests import fake_cache_mix, fake_memory, fake_rank
from tests.fake_cache import decode_rows
from tests.fake_cache_mix import TOPK_MAX as LIST_MAX, refuse_mix
from tests.fake_hip import _n, _p, view
from tests.fake_memory import MAX_KEYS

TOPK_MAX = 1024


def refuse_topk(keys, key_words, N, H, split, h_scale, q_rows, n_rows_max, n_dev, theta, K, s, ld_s, ret_words, ret_idx, n_rows, workspace,
                workspace_bytes, flags):
    if not 1 <= N <= MAX_KEYS or not 1 <= K <= TOPK_MAX or ld_s < K:
        return -1
    if H <= 0 or H % 32 or not (np.isfinite(theta) and theta >= 0) or (split and not (np.isfinite(h_scale) and h_scale > 0)):
        return -1
    if n_rows < 0 or n_rows > 65535 or n_rows_max < 0 or n_rows_max > n_rows:
        return -1
    if n_rows_max == 0:
        return 0
    if not all(_p(x) for x in (keys, key_words, q_rows, s, ret_words, workspace)):
        return -1
    if any(_p(x) % 16 for x in (keys, q_rows, workspace)) or any(_p(x) % 4 for x in (key_words, n_dev, s, ret_words, ret_idx, flags)):
        return -1
    if workspace_bytes < TopkLib.jlm_memory_topk_workspace_bytes(N, n_rows_max, K):
        return -1
    return 0


class TopkLib(fake_cache_mix.MixLib, fake_memory.MemoryLib):
    @staticmethod
    def jlm_memory_topk_workspace_bytes(N, n_rows_max, K):
        if not 1 <= N <= MAX_KEYS or n_rows_max < 0 or not 1 <= K <= TOPK_MAX:
            return 0
        return n_rows_max * (32 * 4 + K * 8)

    @classmethod
    def jlm_memory_topk_chunk_keys(cls, N, n_rows_max, K, workspace_bytes):
        need = cls.jlm_memory_topk_workspace_bytes(N, n_rows_max, K)
        if not 1 <= N <= MAX_KEYS or n_rows_max < 0 or not 1 <= K <= TOPK_MAX or workspace_bytes < need:
            return 0
        whole = (N + 31) // 32 * 32
        if n_rows_max == 0:
            return whole
        return min(whole, (workspace_bytes - n_rows_max * K * 8) // (n_rows_max * 4) // 32 * 32)

    def jlm_memory_topk(self, keys, key_words, N, H, split, h_scale, q_rows, n_rows_max, n_dev, theta, K, s, ld_s, ret_words, ret_idx, n_rows,
                        workspace, workspace_bytes, flags, stream):
        rc = refuse_topk(keys, key_words, N, H, split, h_scale, q_rows, n_rows_max, n_dev, theta, K, s, ld_s, ret_words, ret_idx, n_rows,
                         workspace, workspace_bytes, flags)
        if rc or n_rows_max == 0:
            return rc
        self.launches.append("memory_topk")
        n = _n(n_rows_max, n_dev)
        if n <= 0:
            return 0
        # (the workspace's content is no part of the contract: a NaN fill makes a reader of anything this call did not write visible)
        view(workspace, workspace_bytes // 4, np.float32)[:] = np.nan
        kv = decode_rows(view(keys, N * H, np.float32).reshape(N, H), split, h_scale)
        kw = view(key_words, N, np.int32)
        qv = decode_rows(view(q_rows, n * H, np.float32).reshape(n, H), split, h_scale)
        sv = view(s, n * ld_s, np.float32).reshape(n, ld_s)
        wv = view(ret_words, K * n_rows, np.int32).reshape(K, n_rows)
        iv = view(ret_idx, K * n_rows, np.int32).reshape(K, n_rows) if _p(ret_idx) else None
        n_q = min(K, N)
        bad = False
        for r in range(n):
            with np.errstate(invalid="ignore", over="ignore"):
                sc = (float(np.float32(theta)) * (kv @ qv[r])).astype(np.float32) + np.float32(0.0)
            bad |= not np.all(np.isfinite(sc))
            order = np.argsort(-sc.astype(np.float64), kind="stable")[:n_q]          # larger first, smaller index first among equals
            sv[r, :n_q], wv[:n_q, r] = sc[order], kw[order]
            if iv is not None:
                iv[:n_q, r] = order
        if bad and _p(flags):
            view(flags, 1, np.int32)[0] |= 1
        return 0

    def jlm_rank_memory_frames(self, m, p, mp, stream, events=None):
        R, S = p.n_rows, p.n_steps
        if R < 0 or S < 0:
            return -1
        split = 1 if m.split_lstm else 0
        V = m.segs[m.n_segs - 1].v_end
        n_q = min(mp.K, mp.N)
        rc = refuse_topk(mp.keys, mp.key_words, mp.N, m.H, split, m.h_scale, p.h[0], R, p.n_live, mp.theta, mp.K, mp.s, mp.ld_s, mp.ret_words,
                         mp.ret_idx, R, mp.workspace, mp.workspace_bytes, mp.flags)
        rc = rc or refuse_mix(p.logits, p.ld_logits, V, mp.s, mp.ld_s, mp.ret_words, mp.K, R, R, p.n_live, n_q, mp.first, mp.K, mp.lam, None,
                              mp.flags)
        if rc:
            return rc
        if mp.keep_idx and not _p(mp.ret_idx):
            return -1
        if not 0 <= mp.top_k <= min(LIST_MAX, V) or (mp.top_k and not (_p(mp.top_ids) and _p(mp.top_nll) and p.n_live_host)):
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
        self.launches.append("rank_memory_frames")
        at = lambda base, n: _p(base) + 4 * n
        for t in range(S):
            bound = int(p.n_live_host[t]) if p.n_live_host else R
            if bound == 0:
                continue
            ndev = at(p.n_live, t)
            h_in, h_out, c_in, c_out = p.h[t & 1], p.h[(t + 1) & 1], p.c[t & 1], p.c[(t + 1) & 1]
            rc = self._step(m, h_in, c_in, h_out, c_out, p.T, p.rows, p.prev0 if t == 0 else p.rows, at(p.word, t * R), bound, ndev, p.logits,
                            p.ld_logits, stream)
            idx = at(mp.ret_idx, t * mp.K * R) if mp.keep_idx else mp.ret_idx
            rc = rc or self.jlm_memory_topk(mp.keys, mp.key_words, mp.N, m.H, split, m.h_scale, h_out, bound, ndev, mp.theta, mp.K, mp.s, mp.ld_s,
                                            mp.ret_words, idx, R, mp.workspace, mp.workspace_bytes, mp.flags, stream)
            rc = rc or self.jlm_cache_mix_rows(p.logits, p.ld_logits, V, m.self_norm, mp.s, mp.ld_s, mp.ret_words, mp.K, R, bound, ndev, n_q,
                                               mp.first, mp.K, mp.lam, None, mp.flags, stream)
            rc = rc or self.jlm_rank_rows(p.logits, p.ld_logits, V, bound, ndev, at(p.target, t * R), p.ids, p.n_ids, p.lv_off, p.lv_lo,
                                          p.lv_hi, p.n_levels, at(p.rank, t * R * (p.n_levels + 1)), p.flags, stream)
            if not rc and mp.top_k:
                rc = self.jlm_topk_rows(p.logits, p.ld_logits, V, bound, mp.top_k, m.self_norm, at(mp.top_ids, t * R * mp.top_k),
                                        _p(mp.top_nll) + 8 * t * R * mp.top_k, mp.top_k, p.flags, stream)
            if rc:
                return rc
        return 0

    def jlm_predict_memory_rows(self, m, p, stream, sets=None):
        R = p.n_rows
        if R < 0 or not all(_p(x) for x in (p.rows, p.logits, p.ids, p.nll)):
            return -1
        if m.untied and m.split_lstm:
            return -2
        split = 1 if m.split_lstm else 0
        V = m.segs[m.n_segs - 1].v_end
        n_q = min(p.K, p.N)
        rc = refuse_topk(p.keys, p.key_words, p.N, m.H, split, m.h_scale, p.h, R, None, p.theta, p.K, p.s, p.ld_s, p.ret_words, p.ret_idx, R,
                         p.workspace, p.workspace_bytes, p.memory_flags)
        rc = rc or refuse_mix(p.logits, p.ld_logits, V, p.s, p.ld_s, p.ret_words, p.K, R, R, None, n_q, p.first, p.K, p.lam, None, p.memory_flags)
        if rc or not 1 <= p.k <= min(LIST_MAX, V):
            return rc or -1
        if R == 0:
            return 0
        if not _p(p.T) and not (bool(m.untied) and not m.split_lstm):
            return -1
        self.launches.append("predict_memory_rows")
        rc = self._step(m, None, None, p.h, None, p.T, p.rows, None, None, R, None, p.logits, p.ld_logits, stream, lstm=False)
        rc = rc or self.jlm_memory_topk(p.keys, p.key_words, p.N, m.H, split, m.h_scale, p.h, R, None, p.theta, p.K, p.s, p.ld_s, p.ret_words,
                                        p.ret_idx, R, p.workspace, p.workspace_bytes, p.memory_flags, stream)
        rc = rc or self.jlm_cache_mix_rows(p.logits, p.ld_logits, V, m.self_norm, p.s, p.ld_s, p.ret_words, p.K, R, R, None, n_q, p.first, p.K,
                                           p.lam, None, p.memory_flags, stream)
        return rc or self.jlm_topk_rows(p.logits, p.ld_logits, V, R, p.k, m.self_norm, p.ids, p.nll, p.k, p.flags, stream, sets=sets)


class TopkOps(fake_cache_mix.MixOps, fake_memory.MemoryOps):
    def __init__(self, lib=None):
        fake_cache_mix.MixOps.__init__(self, lib or TopkLib())

    def memory_topk(self, keys, key_words, N, H, split, h_scale, q_rows, n_rows, theta, K, s, ld_s, ret_words, ret_idx, workspace, flags):
        o = self._o
        R = int(n_rows)
        assert keys.numel() >= N * H and key_words.numel() >= N and q_rows.numel() >= R * H and s.numel() >= R * ld_s
        assert ret_words.numel() >= K * R and ret_idx.numel() >= K * R
        self._chk(self.lib.jlm_memory_topk(o(keys), o(key_words), int(N), int(H), int(bool(split)), float(h_scale), o(q_rows), R, None,
                                           float(theta), int(K), o(s), int(ld_s), o(ret_words), o(ret_idx), R, o(workspace),
                                           workspace.numel() * 4, o(flags), 0), "jlm_memory_topk")

    def _mix_plan(self, mp, m, R, keys, key_words, N, theta, lam, K, s, ld_s, ret_words, ret_idx, first, workspace):
        o = self._o
        assert keys.numel() >= N * m.H and key_words.numel() >= N and s.numel() >= R * ld_s and ret_words.numel() >= K * R and first.numel() >= R
        mp.keys, mp.key_words, mp.N, mp.theta, mp.lam, mp.K = o(keys), o(key_words), int(N), float(theta), float(lam), int(K)
        mp.s, mp.ld_s, mp.ret_words, mp.ret_idx, mp.first = o(s), int(ld_s), o(ret_words), o(ret_idx), o(first)
        mp.workspace, mp.workspace_bytes = o(workspace), workspace.numel() * 4

    def rank_memory_frames(self, model, h0, c0, h1, c1, T, logits, ld_logits, rows, prev0, word, target, n_live, n_live_host, ids, lv_off,
                           lv_lo, lv_hi, n_levels, rank, flags, n_rows, n_steps, timed, keys, key_words, N, theta, lam, K, s, ld_s,
                           ret_words, ret_idx, keep_idx, first, workspace, top_k, top_ids, top_nll, mem_flags):
        import torch
        from jlm_amd import _lib
        o, m = self._o, model.m
        R, S = int(n_rows), int(n_steps)
        assert len(n_live_host) == S and all(0 <= x <= R for x in n_live_host)
        assert word.numel() >= S * R and target.numel() >= S * R and rank.numel() >= S * R * (n_levels + 1) and logits.numel() >= R * ld_logits
        assert ret_idx.numel() >= (S if keep_idx else 1) * K * R
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
        mp = _lib.MemoryMixPlan()
        self._mix_plan(mp, m, R, keys, key_words, N, theta, lam, K, s, ld_s, ret_words, ret_idx, first, workspace)
        mp.keep_idx, mp.top_k, mp.top_ids, mp.top_nll, mp.flags = int(bool(keep_idx)), int(top_k), o(top_ids), o(top_nll), o(mem_flags)
        self._chk(self.lib.jlm_rank_memory_frames(m, p, mp, 0, None), "jlm_rank_memory_frames")
        return torch.full((S, 6), 1e-3, dtype=torch.float64) if timed and R > 0 else torch.empty(0, dtype=torch.float64)

    def predict_memory_rows(self, model, h, T, logits, ld_logits, rows, keys, key_words, N, theta, lam, K, s, ld_s, ret_words, ret_idx, first,
                            workspace, k, mask, ld_mask, n_sets, row_set, ids, nll, flags, mem_flags, n_rows):
        from jlm_amd import _lib
        o, m = self._o, model.m
        R = int(n_rows)
        if m.untied and m.split_lstm:
            raise RuntimeError("jlm.predict_memory_rows: an untied split-row model has no one-step form")
        assert h.numel() >= R * m.H and logits.numel() >= R * ld_logits and ids.numel() >= R * k and nll.numel() >= R * k
        sets = None
        if mask is not None:
            assert len(row_set) == R and all(-1 <= x < n_sets for x in row_set)
            bits = mask.numpy().view(np.uint32).reshape(-1)[:n_sets * ld_mask].reshape(n_sets, ld_mask)
            V = m.segs[m.n_segs - 1].v_end
            member = lambda q: np.flatnonzero((bits[q][np.arange(V) >> 5] >> (np.arange(V) & 31).astype(np.uint32)) & 1)
            sets = [None if q < 0 else member(q) for q in row_set]
        p = _lib.PredictMemoryPlan()
        p.n_rows, p.h, p.T, p.logits, p.ld_logits, p.rows = R, o(h), o(T), o(logits), int(ld_logits), o(rows)
        self._mix_plan(p, m, R, keys, key_words, N, theta, lam, K, s, ld_s, ret_words, ret_idx, first, workspace)
        p.k, p.ids, p.nll, p.flags, p.memory_flags = int(k), o(ids), o(nll), o(flags), o(mem_flags)
        self._chk(self.lib.jlm_predict_memory_rows(m, p, 0, sets=sets), "jlm_predict_memory_rows")


def install(monkeypatch):
    """fake_memory.install with the doubles above"""
    import torch
    from jlm_amd import _lib, ops

    fake = TopkLib()
    monkeypatch.setattr(_lib, "lib", lambda: fake)
    monkeypatch.setattr(_lib, "require_gpu", lambda: torch.device("cpu"))
    monkeypatch.setattr(ops, "_backend", TopkOps(fake))
    return fake
