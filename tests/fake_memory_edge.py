"""The numpy double of ``jlm_memory_gather_rows`` / ``jlm_memory_cell_patch``, of ``jlm_decode_plan.memory`` inside ``jlm_decode_frames``
and of ``torch.ops.jlm.seed_memory`` / ``clear_memory`` / ``decode_frames`` for the CPU-only suite:
tests/fake_memory_topk.py's classes and the entry points more (the existing doubles stay as they are).  TEST INFRASTRUCTURE ONLY; it
restates the contract written in include/jlm_hip.h, not the HIP code.

The frame loop of tests/fake_hip.py has no plug, so the memory's three launches of frame f -- gather, retrieval, patch, behind the
frame's normaliser -- run in front of the beam step of frame f + 1, which is where the C loop's order puts them; the patch folds the
pending normaliser slices, and the beam step then runs unfused, as in the C loop.  Every launcher a frame loop calls is recorded in
``launches`` (``frame_log``), so that a test can hold two loops' launch lists against each other."""
import ctypes
import inspect

import numpy as np

from tests import fake_memory_topk
from tests.fake_hip import _n, _p, view
from tests.fake_memory_topk import TOPK_MAX, refuse_topk

MAX_BEAM = 1024
# the launchers jlm_decode_frames may call (tests/fake_hip.py FakeLib.jlm_decode_frames): recorded by name while a frame loop runs
FRAME_CALLS = ("jlm_wordlist_merge_split", "jlm_wordlist_lse", "jlm_wordlist_lse_split", "jlm_wordlist_lse_perm", "jlm_lstm_step",
               "jlm_lstm_step_xg", "jlm_gemm_nt", "jlm_gemm_nt_split", "jlm_pack_t_mixed", "jlm_pack_t_mixed6", "jlm_edge_logits_perm",
               "jlm_vocab_lse_partials", "jlm_vocab_lse_partials_split", "jlm_vocab_lse_mixed", "jlm_vocab_lse_hybrid",
               "jlm_vocab_lse_split", "jlm_vocab_lse_stationary", "jlm_backtrace")


def refuse_gather(h, H, n_pool_rows, rows, n_dev, n_rows_max, out):
    if H <= 0 or H % 4 or n_pool_rows < 0 or not 0 <= n_rows_max <= 65535:
        return -1
    if n_rows_max == 0:
        return 0
    if not (_p(h) and _p(rows) and _p(out)) or n_pool_rows < 1:
        return -1
    if _p(h) % 16 or _p(out) % 16 or _p(rows) % 4 or _p(n_dev) % 4:
        return -1
    return 0


def refuse_patch(s, ld_s, ret_words, n_rows, N, K, lam, cnt, sent_len, frame, n_sent, beam, wl, wl_off, wl_idx, wl_base, wl_out, edge, part,
                 ld_part, n_parts, live_base, lse, flags):
    if n_sent < 0 or frame < 0 or not 1 <= beam <= MAX_BEAM:
        return -1
    if N < 1 or not 1 <= K <= TOPK_MAX or ld_s < K or not 1 <= n_rows <= 65535 or n_sent > 65535:
        return -1
    lam = float(np.float32(lam))
    if not 0.0 < lam < 1.0:
        return -1
    if _p(part) and (not _p(lse) or n_parts < 1 or ld_part < 1):
        return -1
    if n_sent == 0:
        return 0
    if not all(_p(x) for x in (s, ret_words, cnt, sent_len, wl, wl_off, wl_idx, wl_out, edge, live_base)) or wl_base < 0:
        return -1
    if any(_p(x) % 4 for x in (s, edge, flags, ret_words)) or _p(part) % 8 or _p(lse) % 8:
        return -1
    return 0


class EdgeLib(fake_memory_topk.TopkLib):
    def __init__(self):
        super().__init__()
        self._loop = None               # (m, p, lat, memory) of the frame loop that is running
        for name in FRAME_CALLS:
            if hasattr(type(self), name):
                setattr(self, name, self._logged(name))

    def _logged(self, name):
        static = isinstance(inspect.getattr_static(type(self), name), staticmethod)
        fn = getattr(type(self), name)

        def call(*a, **kw):
            if self._loop is not None:
                self.launches.append(name[4:])
            return fn(*a, **kw) if static else fn(self, *a, **kw)
        return call

    def frame_log(self):
        """the launches recorded so far, and a fresh list"""
        out, self.launches = self.launches, []
        return out

    # ------------------------------------------------------------------ the two launchers
    jlm_memory_gather_rows_refuse = staticmethod(refuse_gather)
    jlm_memory_cell_patch_refuse = staticmethod(refuse_patch)

    def jlm_memory_gather_rows(self, h, H, n_pool_rows, rows, n_dev, n_rows_max, out, stream):
        rc = refuse_gather(h, H, n_pool_rows, rows, n_dev, n_rows_max, out)
        if rc or n_rows_max == 0:
            return rc
        self.launches.append("memory_gather_rows")
        n = _n(n_rows_max, n_dev)
        if n <= 0:
            return 0
        pool = view(h, n_pool_rows * H, np.float32).reshape(n_pool_rows, H)
        dst = view(out, n_rows_max * H, np.float32).reshape(n_rows_max, H)
        idx = view(rows, n, np.int32)
        for i in range(n):
            if 0 <= idx[i] < n_pool_rows:
                dst[i] = pool[idx[i]]          # (raw 4-byte values: either state-row format)
        return 0

    def jlm_memory_cell_patch(self, s, ld_s, ret_words, n_rows, N, K, lam, cnt, sent_len, frame, n_sent, beam, wl, wl_off, wl_idx, wl_base,
                              wl_out, edge, part, ld_part, n_parts, live_base, lse, flags, stream):
        rc = refuse_patch(s, ld_s, ret_words, n_rows, N, K, lam, cnt, sent_len, frame, n_sent, beam, wl, wl_off, wl_idx, wl_base, wl_out, edge,
                          part, ld_part, n_parts, live_base, lse, flags)
        if rc or n_sent == 0:
            return rc
        self.launches.append("memory_cell_patch")
        lam = float(np.float32(lam))
        log1m, log_rho = np.log1p(-lam), np.log(lam) - np.log1p(-lam)
        n_q = min(K, N)
        cntv, slen, basev = view(cnt, n_sent, np.int32), view(sent_len, n_sent, np.int32), view(live_base, n_sent, np.int32)
        sv = view(s, n_rows * ld_s, np.float32).reshape(n_rows, ld_s)
        wv = view(ret_words, K * n_rows, np.int32).reshape(K, n_rows)
        fl = view(flags, 1, np.int32) if _p(flags) else None
        pv = view(part, n_parts * ld_part * 2, np.float32).reshape(n_parts, ld_part, 2).astype(np.float64) if _p(part) else None
        idxv = view(wl_idx, n_sent, np.int32)
        for j in range(n_sent):
            kcnt = min(int(cntv[j]), beam)
            if frame >= slen[j] or kcnt <= 0:
                continue
            base = int(basev[j])
            L = np.zeros(kcnt)
            if pv is not None:
                ls = view(_p(lse) + 8 * j * beam, kcnt, np.float64)
                for k in range(kcnt):
                    q = pv[:, base + k]
                    with np.errstate(all="ignore"):
                        mx = q[:, 0].max()
                        l = mx + np.log((q[:, 1] * np.exp(q[:, 0] - mx)).sum())
                    if not abs(l) < 1.0e300:
                        if fl is not None:
                            fl[0] |= 1
                        l = 1.0e30
                    ls[k] = L[k] = l
            li = wl_base + int(idxv[j])
            off = view(_p(wl_off) + 4 * li, 2, np.int32)
            a, J = int(off[0]), int(off[1] - off[0])
            words = view(_p(wl) + 4 * a, J, np.int32) if J else np.zeros(0, dtype=np.int32)
            outs = view(_p(wl_out) + 4 * a, J, np.int32) if J else words
            for k in range(kcnt):
                c = base + k
                if not 0 <= c < n_rows:
                    continue
                sc = sv[c, :n_q]
                if not np.all(np.isfinite(sc)):
                    if fl is not None:
                        fl[0] |= 8
                    continue
                e = np.exp(sc - sc.max()).astype(np.float32)             # (f32 sums, in list order)
                Z = np.float32(0.0)
                for x in e:
                    Z = np.float32(Z + x)
                lw = wv[:n_q, c]
                for p in range(J):
                    cell = view(_p(edge) + 4 * (int(outs[p]) * beam + k), 1, np.float32)
                    y = float(cell[0])
                    hit = lw == words[p]
                    if hit.any():
                        M = np.float32(0.0)
                        for x in e[hit]:
                            M = np.float32(M + x)
                        with np.errstate(divide="ignore"):
                            cell[0] = L[k] + log1m + np.logaddexp(y - L[k], (log_rho + np.log(float(M))) - np.log(float(Z)))
                    else:
                        cell[0] = y + log1m
        return 0

    # ------------------------------------------------------------------ the frame loop
    def jlm_decode_frames(self, m, p, lat, st, stream, side_stream, events=None):
        from jlm_amd import _lib
        mem = _lib.DecodeMemory.from_address(_p(p.memory)) if _p(p.memory) else None
        B, beam, F = lat.n_sent, lat.beam, lat.n_frames
        rmax = B * beam
        if mem is not None:
            # every refusal before the first launch
            if _p(p.cache) or _p(p.ngram) or p.kind != 0 or not _p(st.live_base) or (not m.self_norm and (not _p(p.part) or p.max_parts < 1)) \
                    or rmax > 65535:
                return -1
            split = 1 if m.split_lstm else 0
            rc = refuse_gather(p.h, m.H, F * rmax, st.live, st.n_live, rmax, mem.q_rows)
            rc = rc or refuse_topk(mem.keys, mem.key_words, mem.N, m.H, split, m.h_scale, mem.q_rows, rmax, st.n_live, mem.theta, mem.K, mem.s,
                                   mem.ld_s, mem.ret_words, None, rmax, mem.workspace, mem.workspace_bytes, mem.flags)
            rc = rc or refuse_patch(mem.s, mem.ld_s, mem.ret_words, rmax, mem.N, mem.K, mem.lam, st.cnt, lat.sent_len, 0, B, beam, p.sg_word,
                                    p.sg_off, p.sidx, 0, p.sg_node, p.edge, None if m.self_norm else p.part, rmax, 1, st.live_base, st.lse,
                                    st.flags)
            if rc:
                return rc
        self._loop = (m, p, lat, mem)
        try:
            return super().jlm_decode_frames(m, p, lat, st, stream, side_stream, events)
        finally:
            self._loop = None

    def jlm_beam_step(self, lat, st, frame, mode, max_cands, stream):
        loop = self._loop
        if loop is not None and loop[3] is not None and frame >= 1:
            m, p, _lat, mem = loop
            B, beam, F = lat.n_sent, lat.beam, lat.n_frames
            rmax, f = B * beam, frame - 1
            cell, bound = f * B, (B if f == 0 else rmax)
            at = lambda base, n, size=4: _p(base) + size * n
            rows, ndev = at(st.live, f * rmax), at(st.n_live, f)
            pending = st.n_parts if _p(st.lse_part) else 0
            rc = self.jlm_memory_gather_rows(p.h, m.H, F * rmax, rows, ndev, bound, mem.q_rows, stream)
            rc = rc or self.jlm_memory_topk(mem.keys, mem.key_words, mem.N, m.H, 1 if m.split_lstm else 0, m.h_scale, mem.q_rows, bound, ndev,
                                            mem.theta, mem.K, mem.s, mem.ld_s, mem.ret_words, None, rmax, mem.workspace, mem.workspace_bytes,
                                            mem.flags, stream)
            rc = rc or self.jlm_memory_cell_patch(mem.s, mem.ld_s, mem.ret_words, rmax, mem.N, mem.K, mem.lam, at(st.cnt, cell), lat.sent_len, f,
                                                  B, beam, p.sg_word, p.sg_off, p.sidx, cell, p.sg_node, p.edge,
                                                  st.lse_part if pending else None, rmax, pending, at(st.live_base, cell),
                                                  at(st.lse, f * rmax, 8), st.flags, stream)
            if rc:
                return rc
            st.lse_part, st.n_parts = None, 0          # folded: the beam step reads lse
        if loop is not None:
            self.launches.append("beam_step")
        return super().jlm_beam_step(lat, st, frame, mode, max_cands, stream)


class EdgeOps(fake_memory_topk.TopkOps):
    def __init__(self, lib=None):
        super().__init__(lib or EdgeLib())

    def seed_memory(self, plan, keys, key_words, N, H, theta, lam, K, q_rows, s, ret_words, workspace, flags):
        import torch
        from jlm_amd import _lib
        rmax = plan.lat.n_sent * plan.lat.beam
        assert N >= 1 and H % 4 == 0 and 1 <= K <= TOPK_MAX and 1 <= rmax <= 65535
        assert keys.numel() >= N * H and key_words.dtype == torch.int32 and key_words.numel() >= N
        assert q_rows.numel() >= rmax * H and s.numel() >= rmax * K and ret_words.numel() >= K * rmax and flags.numel() >= 1
        assert theta >= 0.0 and 0.0 < float(np.float32(lam)) < 1.0
        o = self._o
        mem = plan.mem = _lib.DecodeMemory()
        plan.mem_keep = (keys, key_words, q_rows, s, ret_words, workspace, flags)
        mem.keys, mem.key_words, mem.N, mem.K, mem.theta, mem.lam = o(keys), o(key_words), int(N), int(K), float(theta), float(lam)
        mem.q_rows, mem.s, mem.ld_s, mem.ret_words = o(q_rows), o(s), s.numel() // rmax, o(ret_words)
        mem.workspace, mem.workspace_bytes, mem.flags = o(workspace), workspace.numel() * 4, o(flags)
        plan.p.memory = ctypes.addressof(mem)

    def clear_memory(self, plan):
        plan.p.memory = None
        plan.mem = plan.mem_keep = None

    def decode_frames(self, model, plan, *a, **kw):
        try:
            return super().decode_frames(model, plan, *a, **kw)
        finally:
            plan.p.memory = None               # (seed_memory: the memory of ONE frame loop)


def install(monkeypatch):
    """fake_memory_topk.install with the doubles above"""
    import torch
    from jlm_amd import _lib, ops

    fake = EdgeLib()
    monkeypatch.setattr(_lib, "lib", lambda: fake)
    monkeypatch.setattr(_lib, "require_gpu", lambda: torch.device("cpu"))
    monkeypatch.setattr(ops, "_backend", EdgeOps(fake))
    return fake
