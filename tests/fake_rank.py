"""The numpy double of ``jlm_rank_rows`` / ``jlm_rank_frames`` and of ``torch.ops.jlm.rank_rows`` / ``rank_frames`` for the CPU-only
suite: tests/fake_hip.py's FakeLib and FakeOps with the two entry points more (that file stays as it is).  TEST INFRASTRUCTURE ONLY; it
restates the contract written in include/jlm_hip.h, not the HIP code.
"""
import ctypes

import numpy as np

from tests import fake_hip
from tests.fake_hip import _n, _p, view

MAX_LEVELS = 32


def rank_in(y, t, members):
    """the header's rank(S) of target t in the f32 row y: S = the word ids ``members`` (ids outside the row are no words)"""
    w = np.asarray(members, dtype=np.int64)
    w = w[(w >= 0) & (w < len(y))]
    with np.errstate(invalid="ignore"):
        v = y[w]
        return int(np.count_nonzero(v > y[t]) + np.count_nonzero((v == y[t]) & (w < t)))


class RankLib(fake_hip.FakeLib):
    def __init__(self):
        self.launches = []                # the entry points called, in order (a refused call launches nothing)

    def jlm_rank_rows(self, y, ld_y, n_cols, n_rows_max, n_dev, target, ids, n_ids, lv_off, lv_lo, lv_hi, n_levels, rank, flags, stream):
        if n_cols < 1 or ld_y % 4 or ld_y < (n_cols + 3) // 4 * 4 or not _p(y) or _p(y) % 16:
            return -1
        if not 0 <= n_levels <= MAX_LEVELS or not _p(target) or not _p(rank):
            return -1
        if _p(lv_off) and (n_ids < 0 or not _p(lv_lo) or not _p(lv_hi) or (n_ids > 0 and not _p(ids))):
            return -1
        if n_rows_max <= 0:
            return 0
        self.launches.append("rank_rows")
        n = _n(n_rows_max, n_dev)
        if n <= 0:
            return 0
        yv = view(y, n * ld_y, np.float32).reshape(n, ld_y)
        tg = view(target, n, np.int32)
        out = view(rank, n * (n_levels + 1), np.int32).reshape(n, n_levels + 1)
        idv = view(ids, n_ids, np.int32) if _p(lv_off) and n_ids > 0 else np.zeros(0, np.int32)
        off = view(lv_off, n_cols + 1, np.int32) if _p(lv_off) else None
        fl = 0
        for r in range(n):
            t = int(tg[r])
            out[r] = -1
            if not 0 <= t < n_cols:
                fl |= 2
                continue
            row = yv[r, :n_cols]
            if np.isnan(row[t]):
                fl |= 1
                continue
            out[r, 0] = rank_in(row, t, np.arange(n_cols))
            if off is None:
                continue
            e0 = int(off[t])
            for i in range(min(max(int(off[t + 1]) - e0, 0), n_levels)):
                lo = max(int(view(_p(lv_lo) + 4 * (e0 + i), 1, np.int32)[0]), 0)
                hi = min(int(view(_p(lv_hi) + 4 * (e0 + i), 1, np.int32)[0]), n_ids)
                out[r, 1 + i] = rank_in(row, t, idv[lo:hi] if hi > lo else [])
        if fl and _p(flags):
            view(flags, 1, np.int32)[0] |= fl
        return 0

    def jlm_rank_frames(self, m, p, stream, events=None):
        """per step: the LSTM step and the T projection of the live rows, jlm_gemm_nt per segment into plan.logits (+ b2), jlm_rank_rows"""
        R, S = p.n_rows, p.n_steps
        if R < 0 or S < 0 or not all(_p(x) for x in (p.rows, p.prev0, p.word, p.target, p.n_live, p.logits, p.rank)):
            return -1
        if not 0 <= p.n_levels <= MAX_LEVELS:
            return -1
        if R == 0 or S == 0:
            return 0
        t_is_state = bool(m.untied) and not m.split_lstm
        if m.split_lstm and not m.wt8:
            return -2
        if not _p(p.T) and not t_is_state:
            return -1
        V = m.segs[m.n_segs - 1].v_end
        if p.ld_logits % 4 or p.ld_logits < (V + 3) // 4 * 4:
            return -1
        at = lambda base, n: _p(base) + 4 * n
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
                rc = self.jlm_gemm_nt(at(T, sg.t_off), m.ldt, None, sg.B, sg.ldb, None, at(p.logits, sg.v_start), p.ld_logits, None,
                                      at(m.b2, sg.v_start), bound, sg.v_end - sg.v_start, sg.k, None, stream)
                if rc:
                    return rc
            rc = self.jlm_rank_rows(p.logits, p.ld_logits, V, bound, ndev, at(p.target, t * R), p.ids, p.n_ids, p.lv_off, p.lv_lo, p.lv_hi,
                                    p.n_levels, at(p.rank, t * R * (p.n_levels + 1)), p.flags, stream)
            if rc:
                return rc
        return 0


class RankOps(fake_hip.FakeOps):
    def __init__(self, lib=None):
        fake_hip.FakeOps.__init__(self, lib or RankLib())

    @staticmethod
    def _levels(ids, lv_off, lv_lo, lv_hi, n_cols, n_levels):
        if lv_off is None:
            return None, 0, None, None, None
        assert lv_off.numel() >= n_cols + 1 and lv_lo.numel() == lv_hi.numel()
        o = fake_hip.FakeOps._o
        return (o(ids) if ids.numel() else None, int(ids.numel()), o(lv_off), o(lv_lo) if lv_lo.numel() else o(lv_off),
                o(lv_hi) if lv_hi.numel() else o(lv_off))

    def rank_rows(self, y, ld, n_cols, n_rows, n_dev, target, ids, lv_off, lv_lo, lv_hi, n_levels, rank, flags):
        o = self._o
        idp, n_ids, off, lo, hi = self._levels(ids, lv_off, lv_lo, lv_hi, n_cols, n_levels)
        assert rank.numel() >= n_rows * (n_levels + 1) and target.numel() >= n_rows
        self._chk(self.lib.jlm_rank_rows(o(y), int(ld), int(n_cols), int(n_rows), o(n_dev), o(target), idp, n_ids, off, lo, hi, int(n_levels),
                                         o(rank), o(flags), 0), "jlm_rank_rows")

    def rank_frames(self, model, h0, c0, h1, c1, T, logits, ld_logits, rows, prev0, word, target, n_live, n_live_host, ids, lv_off, lv_lo,
                    lv_hi, n_levels, rank, flags, n_rows, n_steps, timed):
        import torch
        from jlm_amd import _lib
        o, m = self._o, model.m
        R, S = int(n_rows), int(n_steps)
        assert len(n_live_host) == S and all(0 <= x <= R for x in n_live_host)
        assert word.numel() >= S * R and target.numel() >= S * R and rank.numel() >= S * R * (n_levels + 1) and logits.numel() >= R * ld_logits
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
        self._chk(self.lib.jlm_rank_frames(m, p, 0, None), "jlm_rank_frames")
        return torch.full((S, 4), 1e-3, dtype=torch.float64) if timed and R > 0 else torch.empty(0, dtype=torch.float64)


def install(monkeypatch):
    """fake_hip.install with the doubles above"""
    import torch
    from jlm_amd import _lib, ops

    fake = RankLib()
    monkeypatch.setattr(_lib, "lib", lambda: fake)
    monkeypatch.setattr(_lib, "require_gpu", lambda: torch.device("cpu"))
    monkeypatch.setattr(ops, "_backend", RankOps(fake))
    return fake
