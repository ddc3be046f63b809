"""The numpy double of ``jlm_memory_rows`` / ``jlm_memory_workspace_bytes`` / ``jlm_score_memory_frames`` and of
``torch.ops.jlm.score_memory_frames`` -- and of the plain ``jlm_score_frames`` / ``score_frames``, which the memory's results are
compared with bit for bit -- for the CPU-only suite: tests/fake_cache.py's CacheLib and CacheOps with the entry points more
(that file stays as it is).  TEST INFRASTRUCTURE ONLY; it restates the contract written in include/jlm_hip.h, not the HIP code.
"""
import ctypes

import numpy as np

from tests import fake_cache
from tests.fake_cache import MAX_THETAS, decode_rows
from tests.fake_hip import _p, view

MAX_KEYS = 1 << 24
MIN_SPLIT_KEYS = 512
MAX_SPLITS = 128


def keys_per_split(N):
    """S of the header: max(512, ceil(ceil(N / 128) / 64) * 64); 0 for N outside [1, 2^24]"""
    if not 1 <= N <= MAX_KEYS:
        return 0
    per = (N + MAX_SPLITS - 1) // MAX_SPLITS
    return max(MIN_SPLIT_KEYS, (per + 63) // 64 * 64)


class MemoryLib(fake_cache.CacheLib):
    @staticmethod
    def jlm_memory_keys_per_split(N):
        return keys_per_split(N)

    @staticmethod
    def jlm_memory_workspace_bytes(N, n_rows, n_steps, n_theta):
        if not 1 <= N <= MAX_KEYS or n_rows < 0 or n_steps < 0 or n_theta < 1:
            return 0
        S = keys_per_split(N)
        return n_theta * ((N + S - 1) // S) * 3 * n_rows * n_steps * 4

    @classmethod
    def _refuse_memory(cls, keys, key_words, N, H, split, h_scale, q_rows, q_words, n_rows, n_steps, length, thetas, n_theta, lpm, workspace,
                       workspace_bytes, flags):
        if n_rows < 0 or n_steps < 0 or not 1 <= N <= MAX_KEYS:
            return -1
        if H <= 0 or H % 32:
            return -1
        if not 1 <= n_theta <= MAX_THETAS or thetas is None:
            return -1
        if any(not (np.isfinite(thetas[t]) and thetas[t] >= 0) for t in range(n_theta)):
            return -1
        if split and not (np.isfinite(h_scale) and h_scale > 0):
            return -1
        if n_rows == 0 or n_steps == 0:
            return 0
        if n_rows > 65535 or n_rows * n_steps >= 1 << 27:
            return -1
        if not all(_p(x) for x in (keys, key_words, q_rows, q_words, lpm, workspace)):
            return -1
        if _p(keys) % 16 or _p(q_rows) % 16 or any(_p(x) % 4 for x in (key_words, q_words, length, lpm, workspace, flags)):
            return -1
        if workspace_bytes < cls.jlm_memory_workspace_bytes(N, n_rows, n_steps, n_theta):
            return -1
        return 0

    def jlm_memory_rows(self, keys, key_words, N, H, split, h_scale, q_rows, q_words, n_rows, n_steps, length, thetas, n_theta, lpm, workspace,
                        workspace_bytes, flags, stream):
        rc = self._refuse_memory(keys, key_words, N, H, split, h_scale, q_rows, q_words, n_rows, n_steps, length, thetas, n_theta, lpm,
                                 workspace, workspace_bytes, flags)
        if rc or n_rows == 0 or n_steps == 0:
            return rc
        self.launches.append("memory_rows")
        kv = decode_rows(view(keys, N * H, np.float32).reshape(N, H), split, h_scale)
        kw = view(key_words, N, np.int32)
        qraw = view(q_rows, n_steps * n_rows * H, np.float32).reshape(n_steps, n_rows, H)
        qw = view(q_words, n_steps * n_rows, np.int32).reshape(n_steps, n_rows)
        lv = view(length, n_rows, np.int32) if _p(length) else np.full(n_rows, n_steps)
        out = view(lpm, n_theta * n_steps * n_rows, np.float32).reshape(n_theta, n_steps, n_rows)
        # (the workspace's content is no part of the contract: a NaN fill makes a reader of anything this call did not write visible)
        view(workspace, self.jlm_memory_workspace_bytes(N, n_rows, n_steps, n_theta) // 4, np.float32)[:] = np.nan
        bad = False
        for r in range(n_rows):
            for t in range(min(int(lv[r]), n_steps)):
                hq = decode_rows(qraw[t, r], split, h_scale)
                with np.errstate(invalid="ignore", over="ignore"):
                    dot = kv @ hq
                if not np.all(np.isfinite(dot)):
                    bad = True
                    out[:, t, r] = np.nan
                    continue
                out[:, t, r] = -np.inf
                same = kw == qw[t, r]
                if not same.any():
                    continue
                for i in range(n_theta):
                    s = float(np.float32(thetas[i])) * dot
                    e = np.exp(s - s.max())
                    out[i, t, r] = np.log(e[same].sum()) - np.log(e.sum())
        if bad and _p(flags):
            view(flags, 1, np.int32)[0] |= 1
        return 0

    def _steps(self, m, p, hist, words, stream, events=None):
        """jlm_score_frames' steps through the cached loop of tests/fake_cache.py, which restates them: hist [S + 1, R, H] / words
        [S + 1, R] a ring of S + 1 slots (N = 1: cap >= N + S) whose slots 0 .. S - 1 receive the live rows of every written state set
        and the targets; its own cache pass has no query (len = 0) and reads nothing.  The launches it records are taken back."""
        from jlm_amd import _lib
        R, S = p.n_rows, p.n_steps
        first = np.zeros(R, dtype=np.int32)
        length = np.zeros(R, dtype=np.int32)
        lpc = np.zeros((1, S, R), dtype=np.float32)
        zero = (ctypes.c_float * 1)(0.0)
        cp = _lib.CachePlan()
        cp.hist, cp.words, cp.cap, cp.pos0, cp.first, cp.len, cp.N = hist.ctypes.data, words.ctypes.data, S + 1, 0, first.ctypes.data, \
            length.ctypes.data, 1
        cp.thetas, cp.n_theta, cp.lpc, cp.flags = ctypes.cast(zero, ctypes.POINTER(ctypes.c_float)), 1, lpc.ctypes.data, None
        mark = len(self.launches)
        rc = fake_cache.CacheLib.jlm_score_cache_frames(self, m, p, cp, stream, events)
        del self.launches[mark:]
        return rc

    def jlm_score_frames(self, m, p, stream, events=None):
        """the plain loop (include/jlm_hip.h jlm_score_frames): the same steps, nothing kept"""
        R, S = p.n_rows, p.n_steps
        if R < 0 or S < 0 or not all(_p(x) for x in (p.rows, p.prev0, p.word, p.target, p.n_live, p.nll_seq)):
            return -1
        if R == 0 or S == 0:
            return 0
        rc = self._steps(m, p, np.zeros((S + 1, R, m.H), dtype=np.float32), np.zeros((S + 1, R), dtype=np.int32), stream, events)
        if rc == 0:
            self.launches.append("score_frames")
        return rc

    def jlm_score_memory_frames(self, m, p, mp, stream, events=None):
        """jlm_score_frames' steps with the live rows of every written state set and the step's targets kept as the call's queries
        (the store hook of jlm_score_cache_frames over a ring with nothing carried), then jlm_memory_rows"""
        R, S = p.n_rows, p.n_steps
        split = 1 if m.split_lstm else 0
        thetas = [mp.thetas[t] for t in range(max(mp.n_theta, 0))] if mp.thetas else None
        rc = self._refuse_memory(mp.keys, mp.key_words, mp.N, m.H, split, m.h_scale, mp.q_rows, mp.q_words, R, S, mp.len, thetas, mp.n_theta,
                                 mp.lpm, mp.workspace, mp.workspace_bytes, mp.flags)
        if rc:
            return rc
        if R < 0 or S < 0 or not all(_p(x) for x in (p.rows, p.prev0, p.word, p.target, p.n_live, p.nll_seq)):
            return -1
        if R == 0 or S == 0:
            return 0
        # the steps and the store hook are the cached loop's: a ring that starts as the query rows are and goes back into them
        q_rows = view(mp.q_rows, S * R * m.H, np.float32).reshape(S, R, m.H)
        q_words = view(mp.q_words, S * R, np.int32).reshape(S, R)
        hist = np.zeros((S + 1, R, m.H), dtype=np.float32)
        words = np.zeros((S + 1, R), dtype=np.int32)
        hist[:S], words[:S] = q_rows, q_words
        rc = self._steps(m, p, hist, words, stream, events)
        if rc:
            return rc
        self.launches.append("score_memory_frames")
        q_rows[:], q_words[:] = hist[:S], words[:S]
        return self.jlm_memory_rows(mp.keys, mp.key_words, mp.N, m.H, split, m.h_scale, mp.q_rows, mp.q_words, R, S, mp.len, thetas, mp.n_theta,
                                    mp.lpm, mp.workspace, mp.workspace_bytes, mp.flags, stream)


class MemoryOps(fake_cache.CacheOps):
    def __init__(self, lib=None):
        fake_cache.CacheOps.__init__(self, lib or MemoryLib())

    def _score_plan(self, h0, c0, h1, c1, T, Tm, ld_tm, part, max_parts, rows, prev0, word, target, n_live, n_live_host, nll_seq, nll_tok,
                    flags, R, S):
        from jlm_amd import _lib
        o = self._o
        assert len(n_live_host) == S and all(0 <= x <= R for x in n_live_host)
        assert word.numel() >= S * R and target.numel() >= S * R and nll_seq.numel() >= R
        p = _lib.ScorePlan()
        p.n_rows, p.n_steps = R, S
        p.h[0], p.h[1], p.c[0], p.c[1], p.T = o(h0), o(h1), o(c0), o(c1), o(T)
        p.Tm, p.ld_tm, p.part, p.max_parts = o(Tm), int(ld_tm), o(part), int(max_parts)
        p.rows, p.prev0, p.word, p.target, p.n_live = o(rows), o(prev0), o(word), o(target), o(n_live)
        live = (ctypes.c_int * max(S, 1))(*[int(x) for x in n_live_host])
        p.n_live_host = ctypes.cast(live, ctypes.POINTER(ctypes.c_int))
        p.nll_seq, p.nll_tok, p.flags = o(nll_seq), o(nll_tok), o(flags)
        return p, live

    def score_frames(self, model, h0, c0, h1, c1, T, Tm, ld_tm, part, max_parts, rows, prev0, word, target, n_live, n_live_host, nll_seq,
                     nll_tok, flags, n_rows, n_steps, timed):
        import torch
        R, S = int(n_rows), int(n_steps)
        p, _live = self._score_plan(h0, c0, h1, c1, T, Tm, ld_tm, part, max_parts, rows, prev0, word, target, n_live, n_live_host, nll_seq,
                                    nll_tok, flags, R, S)
        self._chk(self.lib.jlm_score_frames(model.m, p, 0, None), "jlm_score_frames")
        return torch.full((S, 4), 1e-3, dtype=torch.float64) if timed and R > 0 else torch.empty(0, dtype=torch.float64)

    def score_memory_frames(self, model, h0, c0, h1, c1, T, Tm, ld_tm, part, max_parts, rows, prev0, word, target, n_live, n_live_host,
                            nll_seq, nll_tok, flags, n_rows, n_steps, timed, keys, key_words, N, q_rows, q_words, length, thetas, lpm,
                            workspace, mem_flags):
        import torch
        from jlm_amd import _lib
        o, m = self._o, model.m
        R, S = int(n_rows), int(n_steps)
        assert 1 <= N <= MAX_KEYS and keys.numel() >= N * m.H and key_words.numel() >= N and keys.element_size() == 4
        assert q_rows.numel() >= S * R * m.H and q_words.numel() >= S * R and lpm.numel() >= len(thetas) * S * R
        assert length.numel() >= R and 1 <= len(thetas) <= MAX_THETAS
        assert workspace.dtype == torch.float32 and workspace.numel() * 4 >= self.lib.jlm_memory_workspace_bytes(N, R, S, len(thetas))
        p, _live = self._score_plan(h0, c0, h1, c1, T, Tm, ld_tm, part, max_parts, rows, prev0, word, target, n_live, n_live_host, nll_seq,
                                    nll_tok, flags, R, S)
        mp = _lib.MemoryPlan()
        mp.keys, mp.key_words, mp.N, mp.q_rows, mp.q_words, mp.len = o(keys), o(key_words), int(N), o(q_rows), o(q_words), o(length)
        th = (ctypes.c_float * len(thetas))(*[float(x) for x in thetas])
        mp.thetas, mp.n_theta = ctypes.cast(th, ctypes.POINTER(ctypes.c_float)), len(thetas)
        mp.lpm, mp.workspace, mp.workspace_bytes, mp.flags = o(lpm), o(workspace), workspace.numel() * 4, o(mem_flags)
        self._chk(self.lib.jlm_score_memory_frames(m, p, mp, 0, None), "jlm_score_memory_frames")
        return torch.full((S, 4), 1e-3, dtype=torch.float64) if timed and R > 0 else torch.empty(0, dtype=torch.float64)


def install(monkeypatch):
    """fake_cache.install with the doubles above"""
    import torch
    from jlm_amd import _lib, ops

    fake = MemoryLib()
    monkeypatch.setattr(_lib, "lib", lambda: fake)
    monkeypatch.setattr(_lib, "require_gpu", lambda: torch.device("cpu"))
    monkeypatch.setattr(ops, "_backend", MemoryOps(fake))
    return fake
