"""The numpy double of ``jlm_cache_rows`` / ``jlm_score_cache_frames`` and of ``torch.ops.jlm.score_cache_frames`` for the CPU-only
suite: tests/fake_hip.py's FakeLib and FakeOps with the entry points more (that file stays as it is).  TEST INFRASTRUCTURE ONLY; it
restates the contract written in include/jlm_hip.h, not the HIP code.
"""
import ctypes

import numpy as np

from tests import fake_hip
from tests.fake_hip import _p, view

MAX_THETAS = 16


def decode_rows(raw, split, h_scale):
    """state rows [..., H] float32 bits -> float64 values in real units (split rows: (hi + lo) / h_scale)"""
    if not split:
        return raw.astype(np.float64)
    H = raw.shape[-1]
    sp = np.ascontiguousarray(raw).view(np.float16).reshape(raw.shape[:-1] + (H // 8, 2, 8)).astype(np.float64)
    with np.errstate(invalid="ignore"):               # (slots nothing was written to hold anything; no window reads them)
        return (sp[..., 0, :] + sp[..., 1, :]).reshape(raw.shape[:-1] + (H,)) / float(h_scale)


class CacheLib(fake_hip.FakeLib):
    def __init__(self):
        self.launches = []                # the entry points called, in order (a refused call launches nothing)

    @staticmethod
    def _refuse(hist, words, cap, n_rows, H, split, h_scale, pos0, n_query, first, length, N, thetas, n_theta, lpc):
        if n_rows < 0 or n_query < 0 or N < 1 or cap < 1 or pos0 < 0 or N + n_query > cap or pos0 + n_query + cap > 0x7fffffff:
            return -1
        if H <= 0 or H % 32:
            return -1
        if not 1 <= n_theta <= MAX_THETAS or thetas is None:
            return -1
        if any(not (np.isfinite(thetas[t]) and thetas[t] >= 0) for t in range(n_theta)):
            return -1
        if split and not (np.isfinite(h_scale) and h_scale > 0):
            return -1
        if n_rows == 0 or n_query == 0:
            return 0
        if n_rows > 65535 or not all(_p(x) for x in (hist, words, first, length, lpc)):
            return -1
        if _p(hist) % 16 or any(_p(x) % 4 for x in (words, first, length, lpc)):
            return -1
        return 0

    def jlm_cache_rows(self, hist, words, cap, n_rows, H, split, h_scale, pos0, n_query, first, length, N, thetas, n_theta, lpc, flags,
                       stream):
        rc = self._refuse(hist, words, cap, n_rows, H, split, h_scale, pos0, n_query, first, length, N, thetas, n_theta, lpc)
        if rc or n_rows == 0 or n_query == 0:
            return rc
        self.launches.append("cache_rows")
        hv = decode_rows(view(hist, cap * n_rows * H, np.float32).reshape(cap, n_rows, H), split, h_scale)
        wv = view(words, cap * n_rows, np.int32).reshape(cap, n_rows)
        fv, lv = view(first, n_rows, np.int32), view(length, n_rows, np.int32)
        out = view(lpc, n_theta * n_query * n_rows, np.float32).reshape(n_theta, n_query, n_rows)
        bad = False
        for r in range(n_rows):
            for q in range(min(int(lv[r]), n_query)):
                qp = pos0 + q
                idx = np.arange(max(qp - N, int(fv[r]), 0), qp)
                out[:, q, r] = -np.inf
                if not len(idx):
                    continue
                with np.errstate(invalid="ignore", over="ignore"):
                    dot = hv[idx % cap, r] @ hv[qp % cap, r]
                if not np.all(np.isfinite(dot)):
                    bad = True
                    out[:, q, r] = np.nan
                    continue
                same = wv[idx % cap, r] == wv[qp % cap, r]
                if not same.any():
                    continue
                for t in range(n_theta):
                    s = float(np.float32(thetas[t])) * dot
                    e = np.exp(s - s.max())
                    out[t, q, r] = np.log(e[same].sum()) - np.log(e.sum())
        if bad and _p(flags):
            view(flags, 1, np.int32)[0] |= 1
        return 0

    def jlm_score_cache_frames(self, m, p, cp, stream, events=None):
        """jlm_score_frames' steps -- the LSTM step and the T projection of the live rows, nll = lse(logits) - logit of the target
        (self_norm: -logit) in float64 -- with the written state rows and the targets copied into the rings, then jlm_cache_rows"""
        R, S = p.n_rows, p.n_steps
        split = 1 if m.split_lstm else 0
        thetas = [cp.thetas[t] for t in range(max(cp.n_theta, 0))] if cp.thetas else None
        rc = self._refuse(cp.hist, cp.words, cp.cap, R, m.H, split, m.h_scale, cp.pos0, S, cp.first, cp.len, cp.N, thetas, cp.n_theta, cp.lpc)
        if rc:
            return rc
        if R < 0 or S < 0 or not all(_p(x) for x in (p.rows, p.prev0, p.word, p.target, p.n_live, p.nll_seq)):
            return -1
        if R == 0 or S == 0:
            return 0
        t_is_state = bool(m.untied) and not m.split_lstm
        if m.split_lstm and not m.wt8:
            return -2
        if not _p(p.T) and not t_is_state:
            return -1
        self.launches.append("score_cache_frames")
        V = m.segs[m.n_segs - 1].v_end
        ld = (V + 3) // 4 * 4
        logits = np.zeros((R, ld), dtype=np.float32)
        at = lambda base, n: _p(base) + 4 * n
        hist = view(cp.hist, cp.cap * R * m.H, np.float32).reshape(cp.cap, R, m.H)
        words = view(cp.words, cp.cap * R, np.int32).reshape(cp.cap, R)
        nll_seq = view(p.nll_seq, R, np.float64)
        nll_tok = view(p.nll_tok, S * R, np.float64).reshape(S, R) if _p(p.nll_tok) else None
        for t in range(S):
            bound = int(p.n_live_host[t]) if p.n_live_host else R
            if bound < 0 or bound > R:
                return -1
            if bound == 0:
                continue
            ndev = at(p.n_live, t)
            h_in, h_out, c_in, c_out = p.h[t & 1], p.h[(t + 1) & 1], p.c[t & 1], p.c[(t + 1) & 1]
            T = h_out if t_is_state else p.T
            prev = p.prev0 if t == 0 else p.rows
            word = at(p.word, t * R)
            if m.split_lstm:
                rc = self.jlm_lstm_step_xg(h_in, c_in, m.H, h_out, c_out, p.rows, prev, word, m.wt8, m.xgate8, m.H, m.gate_descale,
                                           m.h_scale, p.T if m.untied else None, bound, ndev, stream)
            else:
                rc = self.jlm_lstm_step(h_in, c_in, m.H, h_out, c_out, p.rows, prev, word, m.emb, m.ld_emb, m.wt, m.gate_bias, m.kpad,
                                        m.H, m.E, bound, ndev, stream)
            if rc:
                return rc
            if not m.untied:
                if m.split_lstm:
                    rc = self.jlm_gemm_nt_split(h_out, m.H, p.rows, m.pmt_split, m.H, None, T, m.ldt, p.rows, None, m.t_descale, bound,
                                                m.n_t, m.H, ndev, stream)
                else:
                    rc = self.jlm_gemm_nt(h_out, m.H, p.rows, m.pmt, m.H, None, T, m.ldt, p.rows, None, bound, m.n_t, m.H, ndev, stream)
                if rc:
                    return rc
            for i in range(m.n_segs):
                sg = m.segs[i]
                rc = self.jlm_gemm_nt(at(T, sg.t_off), m.ldt, None, sg.B, sg.ldb, None, logits.ctypes.data + 4 * sg.v_start, ld, None,
                                      at(m.b2, sg.v_start), bound, sg.v_end - sg.v_start, sg.k, None, stream)
                if rc:
                    return rc
            tg = view(at(p.target, t * R), R, np.int32)
            for r in range(bound):
                y = logits[r, :V].astype(np.float64)
                top = y.max()
                nll = -y[tg[r]] if m.self_norm else top + np.log(np.exp(y - top).sum()) - y[tg[r]]
                nll_seq[r] += nll
                if nll_tok is not None:
                    nll_tok[t, r] = nll
            slot = (cp.pos0 + t) % cp.cap
            hist[slot, :bound] = view(h_out, R * m.H, np.float32).reshape(R, m.H)[:bound]
            words[slot, :bound] = tg[:bound]
        return self.jlm_cache_rows(cp.hist, cp.words, cp.cap, R, m.H, split, m.h_scale, cp.pos0, S, cp.first, cp.len, cp.N, thetas,
                                   cp.n_theta, cp.lpc, cp.flags, stream)


class CacheOps(fake_hip.FakeOps):
    def __init__(self, lib=None):
        fake_hip.FakeOps.__init__(self, lib or CacheLib())

    def score_cache_frames(self, model, h0, c0, h1, c1, T, Tm, ld_tm, part, max_parts, rows, prev0, word, target, n_live, n_live_host,
                           nll_seq, nll_tok, flags, n_rows, n_steps, timed, hist, words, cap, pos0, first, length, N, thetas, lpc,
                           cache_flags):
        import torch
        from jlm_amd import _lib
        o, m = self._o, model.m
        R, S = int(n_rows), int(n_steps)
        assert len(n_live_host) == S and all(0 <= x <= R for x in n_live_host)
        assert word.numel() >= S * R and target.numel() >= S * R and nll_seq.numel() >= R
        assert hist.numel() >= cap * R * m.H and words.numel() >= cap * R and lpc.numel() >= len(thetas) * S * R
        assert first.numel() >= R and length.numel() >= R and 1 <= len(thetas) <= MAX_THETAS
        p = _lib.ScorePlan()
        p.n_rows, p.n_steps = R, S
        p.h[0], p.h[1], p.c[0], p.c[1], p.T = o(h0), o(h1), o(c0), o(c1), o(T)
        p.Tm, p.ld_tm, p.part, p.max_parts = o(Tm), int(ld_tm), o(part), int(max_parts)
        p.rows, p.prev0, p.word, p.target, p.n_live = o(rows), o(prev0), o(word), o(target), o(n_live)
        live = (ctypes.c_int * max(S, 1))(*[int(x) for x in n_live_host])
        p.n_live_host = ctypes.cast(live, ctypes.POINTER(ctypes.c_int))
        p.nll_seq, p.nll_tok, p.flags = o(nll_seq), o(nll_tok), o(flags)
        cp = _lib.CachePlan()
        cp.hist, cp.words, cp.cap, cp.pos0, cp.first, cp.len, cp.N = o(hist), o(words), int(cap), int(pos0), o(first), o(length), int(N)
        th = (ctypes.c_float * len(thetas))(*[float(x) for x in thetas])
        cp.thetas, cp.n_theta = ctypes.cast(th, ctypes.POINTER(ctypes.c_float)), len(thetas)
        cp.lpc, cp.flags = o(lpc), o(cache_flags)
        self._chk(self.lib.jlm_score_cache_frames(m, p, cp, 0, None), "jlm_score_cache_frames")
        return torch.full((S, 4), 1e-3, dtype=torch.float64) if timed and R > 0 else torch.empty(0, dtype=torch.float64)


def install(monkeypatch):
    """fake_hip.install with the doubles above"""
    import torch
    from jlm_amd import _lib, ops

    fake = CacheLib()
    monkeypatch.setattr(_lib, "lib", lambda: fake)
    monkeypatch.setattr(_lib, "require_gpu", lambda: torch.device("cpu"))
    monkeypatch.setattr(ops, "_backend", CacheOps(fake))
    return fake
