"""The numpy double of ``jlm_alt_head`` / ``jlm_alt_frames`` and of ``torch.ops.jlm.alt_frames`` for the CPU-only suite, and -- so that
the candidate lists can be driven with a left context there too -- of ``jlm_prime_frames`` / ``jlm_seed_context`` and the root rows a
plan with a context steps from: tests/fake_hip.py's FakeLib and FakeOps with the entry points more (that file stays as it is).  TEST
INFRASTRUCTURE ONLY; it restates the contract written in include/jlm_hip.h, not the HIP code.
"""
import ctypes

import numpy as np

from tests import fake_hip
from tests.fake_hip import _p, view


class AltLib(fake_hip.FakeLib):
    def __init__(self):
        self.launches = []                # "alt_head" / "score_step" in the order enqueued (a refused call launches nothing)
        self.fail_alt = None              # an exception jlm_alt_frames raises in place of its work (tests)
        self._root = None                 # (frame 0's row list, ctx_prev, ctx_word) while a decode with a left context runs

    # ------------------------------------------------------------------ left context (include/jlm_hip.h jlm_decode_plan.ctx_prev)
    def jlm_decode_frames(self, m, p, lat, st, stream, side_stream, events=None):
        self._root = (_p(st.live), p.ctx_prev, p.ctx_word) if _p(p.ctx_prev) else None
        try:
            return fake_hip.FakeLib.jlm_decode_frames(self, m, p, lat, st, stream, side_stream, events)
        finally:
            self._root = None

    def _ctx_args(self, rows, prev, word):
        """frame 0 of a plan with a left context reads the root rows' prev / word from ctx_prev / ctx_word"""
        if self._root is not None and _p(rows) == self._root[0]:
            return self._root[1], self._root[2]
        return prev, word

    def jlm_lstm_step(self, h_in, c_in, ld, h_out, c_out, rows, prev, word, *a):
        prev, word = self._ctx_args(rows, prev, word)
        return fake_hip.FakeLib.jlm_lstm_step(self, h_in, c_in, ld, h_out, c_out, rows, prev, word, *a)

    def jlm_lstm_step_xg(self, h_in, c_in, ld, h_out, c_out, rows, prev, word, *a):
        prev, word = self._ctx_args(rows, prev, word)
        return fake_hip.FakeLib.jlm_lstm_step_xg(self, h_in, c_in, ld, h_out, c_out, rows, prev, word, *a)

    def jlm_seed_context(self, src_h, src_c, H, last, has, n_src, idx, n_sent, beam, G, dst_h, dst_c, ctx_prev, ctx_word, stream):
        if n_sent <= 0:
            return 0
        sh, sc = view(src_h, n_src * H, np.float32).reshape(n_src, H), view(src_c, n_src * H, np.float32).reshape(n_src, H)
        dh, dc = view(dst_h, (G + n_sent) * H, np.float32).reshape(-1, H), view(dst_c, (G + n_sent) * H, np.float32).reshape(-1, H)
        lv, hv, iv = view(last, n_src, np.int32), view(has, n_src, np.int32), view(idx, n_sent, np.int32)
        cp, cw = view(ctx_prev, n_sent * beam, np.int32), view(ctx_word, n_sent * beam, np.int32)
        for s in range(n_sent):
            r = int(iv[s])
            if hv[r]:
                dh[G + s], dc[G + s] = sh[r], sc[r]
            cp[s * beam] = G + s if hv[r] else -1
            cw[s * beam] = lv[r]
        return 0

    def _step(self, m, h_in, c_in, h_out, c_out, rows, prev, word, T, bound, ndev):
        """the LSTM step and the T projection of a row set's live prefix (csrc/jlm_decode.hip rows_lstm_step / rows_t_projection)"""
        t_is_state = bool(m.untied) and not m.split_lstm
        if m.split_lstm:
            rc = self.jlm_lstm_step_xg(h_in, c_in, m.H, h_out, c_out, rows, prev, word, m.wt8, m.xgate8, m.H, m.gate_descale, m.h_scale,
                                       T if m.untied else None, bound, ndev, 0)
        else:
            rc = self.jlm_lstm_step(h_in, c_in, m.H, h_out, c_out, rows, prev, word, m.emb, m.ld_emb, m.wt, m.gate_bias, m.kpad, m.H,
                                    m.E, bound, ndev, 0)
        if rc or m.untied:
            return rc
        if m.split_lstm:
            return self.jlm_gemm_nt_split(h_out, m.H, rows, m.pmt_split, m.H, None, T, m.ldt, rows, None, m.t_descale, bound, m.n_t, m.H,
                                          ndev, 0)
        return self.jlm_gemm_nt(h_out, m.H, rows, m.pmt, m.H, None, h_out if t_is_state else T, m.ldt, rows, None, bound, m.n_t, m.H,
                                ndev, 0)

    def jlm_prime_frames(self, m, p, stream):
        R, S = p.n_rows, p.n_steps
        if R <= 0 or S <= 0:
            return 0 if R >= 0 and S >= 0 else -1
        for f in range(S):
            bound = int(p.n_live_host[f])
            if bound < 0 or bound > R:
                return -1
            if bound == 0:
                continue
            args = (p.h[f & 1], p.c[f & 1], m.H, p.h[(f + 1) & 1], p.c[(f + 1) & 1], p.rows, _p(p.prev) + 4 * f * R, _p(p.word) + 4 * f * R)
            if m.split_lstm:
                rc = self.jlm_lstm_step_xg(*args, m.wt8, m.xgate8, m.H, m.gate_descale, m.h_scale, None, bound, _p(p.n_live) + 4 * f, 0)
            else:
                rc = self.jlm_lstm_step(*args, m.emb, m.ld_emb, m.wt, m.gate_bias, m.kpad, m.H, m.E, bound, _p(p.n_live) + 4 * f, 0)
            if rc:
                return rc
        return 0

    # ------------------------------------------------------------------ candidate lists
    @staticmethod
    def jlm_alt_head_refuse(segs, n_segs, b2, ldt, H, mode, a, p):
        if not (1 <= n_segs <= 8) or any(segs[i].k % 4 or segs[i].ldb % 4 or segs[i].t_off % 4 or not _p(segs[i].B) or _p(segs[i].B) % 16
                                         for i in range(n_segs)):
            return -1
        if not (1 <= a.beam <= 1024 and ldt >= 4 and ldt % 4 == 0 and H >= 4 and H % 4 == 0 and a.n_frames >= 1 and mode in (0, 1) and
                0 <= a.rank < a.beam and a.n_sent >= 0 and p.n_rows >= 0 and p.n_steps >= 0):
            return -1
        if a.n_sent == 0 or p.n_rows == 0:
            return 0
        if a.n_frames * a.n_sent * a.beam >= 0x7fffffff:
            return -1
        need = [b2, a.T, a.h, a.c, a.score, a.bp, a.sent_len, a.sent_off, a.sent_rows, a.depth, a.alt, a.prev0, p.h[0], p.c[0], p.nll_seq]
        if not all(_p(x) for x in need) or (mode == 0 and not _p(a.lse)) or _p(a.prev0) != _p(p.prev0) or (p.n_steps > 0 and not _p(p.n_live)):
            return -1
        if any(_p(x) % 16 for x in (a.T, a.h, a.c, p.h[0], p.c[0])) or any(_p(x) % 8 for x in (a.score, a.lse, p.nll_seq)):
            return -1
        if any(_p(x) % 4 for x in (b2, a.bp, a.sent_len, a.sent_off, a.sent_rows, a.depth, a.alt, a.prev0, p.n_live, p.flags)):
            return -1
        if 16 * ldt * 4 + (a.n_frames + 16) * 8 + (a.n_frames + p.n_steps + 2) * 4 > 160 * 1024:
            return -1
        return 0

    def jlm_alt_head(self, segs, n_segs, b2, ldt, H, mode, a, p, stream):
        rc = self.jlm_alt_head_refuse(segs, n_segs, b2, ldt, H, mode, a, p)
        if rc or a.n_sent == 0 or p.n_rows == 0:
            return rc
        self.launches.append("alt_head")
        sg = self._segs(segs, n_segs)
        B, beam, P, R, S = a.n_sent, a.beam, a.n_frames, p.n_rows, p.n_steps
        rmax, G = B * beam, a.n_frames * B * beam
        sc, bp, sl = view(a.score, G, np.float64), view(a.bp, G, np.int32), view(a.sent_len, B, np.int32)
        ls = view(a.lse, G, np.float64) if mode == 0 else None
        off, srows = view(a.sent_off, B + 1, np.int32), view(a.sent_rows, R, np.int32)
        depth, alt = view(a.depth, R, np.int32), view(a.alt, R, np.int32)
        live = view(p.n_live, S, np.int32) if S else np.zeros(0, np.int32)
        prev0, seq = view(a.prev0, R, np.int32), view(p.nll_seq, R, np.float64)
        fl = view(p.flags, 1, np.int32) if _p(p.flags) else np.zeros(1, np.int32)
        sh, sc_ = view(a.h, G * H, np.float32).reshape(G, H), view(a.c, G * H, np.float32).reshape(G, H)
        dh, dc = view(p.h[0], R * H, np.float32).reshape(R, H), view(p.c[0], R * H, np.float32).reshape(R, H)
        for s in range(B):
            i0, i1 = int(off[s]), int(off[s + 1])
            if i0 < 0 or i1 > R or i0 >= i1:
                continue
            L = int(sl[s])
            path, g, ok = [], L * rmax + s * beam + a.rank, 1 <= L < P
            while ok and g != -1:
                if g < 0 or g >= G or len(path) >= P:
                    ok = False
                    break
                path.append(g)
                g = int(bp[g])
            path.reverse()
            K = len(path) - 1 if ok and path else -1
            if K >= 0 and mode == 0 and not np.all(np.abs(ls[path[:K]]) < 1e300):
                fl[0] |= 1
            for r in (int(x) for x in srows[i0:i1]):
                if not 0 <= r < R:
                    continue
                d, j = int(depth[r]), int((live > r).sum())
                if K < 0 or d < 0 or d >= K or d + 1 + j > K:
                    seq[r], prev0[r] = np.inf, -1
                    fl[0] |= 4
                    continue
                w, gd = int(alt[r]), path[d]
                prev0[r] = r
                if not any(x.v_start <= w < x.v_end for x in sg):
                    seq[r] = np.nan
                    fl[0] |= 2
                else:
                    y = self._word_logits(sg, b2, a.T, ldt, gd, 1, [w])[0, 0]
                    with np.errstate(invalid="ignore"):
                        base = sc[gd] + ls[gd] if mode == 0 else sc[gd]
                        seq[r] = (base - np.float64(y)) + (sc[path[K]] - sc[path[d + 1 + j]])
                if j >= 1:
                    dh[r], dc[r] = sh[gd], sc_[gd]
        return 0

    def _score_steps(self, m, p):
        """jlm_score_frames' steps -- the LSTM step and the T projection of the live rows, nll = lse(logits) - logit of the target
        (self_norm: -logit) in float64, added to nll_seq"""
        R, S = p.n_rows, p.n_steps
        if R < 0 or S < 0 or not all(_p(x) for x in (p.rows, p.prev0, p.word, p.target, p.n_live, p.nll_seq)):
            return -1
        if R == 0 or S == 0:
            return 0
        t_is_state = bool(m.untied) and not m.split_lstm
        if m.split_lstm and not m.wt8:
            return -2
        if not _p(p.T) and not t_is_state:
            return -1
        V = m.segs[m.n_segs - 1].v_end
        ld = (V + 3) // 4 * 4
        logits = np.zeros((R, ld), dtype=np.float32)
        at = lambda base, n: _p(base) + 4 * n
        nll_seq = view(p.nll_seq, R, np.float64)
        for t in range(S):
            bound = int(p.n_live_host[t]) if p.n_live_host else R
            if bound < 0 or bound > R:
                return -1
            if bound == 0:
                continue
            self.launches.append("score_step")
            h_out = p.h[(t + 1) & 1]
            T = h_out if t_is_state else p.T
            rc = self._step(m, p.h[t & 1], p.c[t & 1], h_out, p.c[(t + 1) & 1], p.rows, p.prev0 if t == 0 else p.rows,
                            at(p.word, t * R), p.T, bound, at(p.n_live, t))
            if rc:
                return rc
            for i in range(m.n_segs):
                sg = m.segs[i]
                rc = self.jlm_gemm_nt(at(T, sg.t_off), m.ldt, None, sg.B, sg.ldb, None, logits.ctypes.data + 4 * sg.v_start, ld, None,
                                      at(m.b2, sg.v_start), bound, sg.v_end - sg.v_start, sg.k, None, 0)
                if rc:
                    return rc
            tg = view(at(p.target, t * R), R, np.int32)
            for r in range(bound):
                y = logits[r, :V].astype(np.float64)
                top = y.max()
                nll_seq[r] += -y[tg[r]] if m.self_norm else top + np.log(np.exp(y - top).sum()) - y[tg[r]]
        return 0

    def jlm_alt_frames(self, m, a, p, stream, events=None):
        if self.fail_alt is not None:
            raise self.fail_alt
        mode = 1 if m.self_norm else 0
        rc = self.jlm_alt_head_refuse(m.segs, m.n_segs, m.b2, m.ldt, m.H, mode, a, p)
        if rc:
            return rc
        rc = self.jlm_alt_head(m.segs, m.n_segs, m.b2, m.ldt, m.H, mode, a, p, stream)
        if rc or p.n_rows <= 0 or p.n_steps <= 0:
            return rc
        return self._score_steps(m, p)


class _AltPlan(fake_hip._FakePlan):
    def __init__(self, t, i):
        fake_hip._FakePlan.__init__(self, t, i)
        self.H = i.get("H", 0)
        if "ctx_prev" in t:
            self.p.ctx_prev, self.p.ctx_word = t["ctx_prev"].data_ptr(), t["ctx_word"].data_ptr()


class AltOps(fake_hip.FakeOps):
    def __init__(self, lib=None):
        fake_hip.FakeOps.__init__(self, lib or AltLib())
        self.Plan = _AltPlan

    def prime_frames(self, model, h0, c0, h1, c1, rows, prev, word, n_live, n_live_host, n_rows, n_steps):
        from jlm_amd import _lib
        o = self._o
        p = _lib.PrimePlan()
        p.n_rows, p.n_steps = int(n_rows), int(n_steps)
        p.h[0], p.h[1], p.c[0], p.c[1] = o(h0), o(h1), o(c0), o(c1)
        p.rows, p.prev, p.word, p.n_live = o(rows), o(prev), o(word), o(n_live)
        live = (ctypes.c_int * max(int(n_steps), 1))(*[int(x) for x in n_live_host])
        p.n_live_host = ctypes.cast(live, ctypes.POINTER(ctypes.c_int))
        self._chk(self.lib.jlm_prime_frames(model.m, p, 0), "jlm_prime_frames")

    def seed_context(self, plan, src_h, src_c, last, has, idx):
        assert plan.H > 0 and plan.p.ctx_prev and plan.p.ctx_word
        G = plan.frames * plan.lat.n_sent * plan.lat.beam
        self._chk(self.lib.jlm_seed_context(self._o(src_h), self._o(src_c), plan.H, self._o(last), self._o(has), int(last.numel()),
                                            self._o(idx), plan.lat.n_sent, plan.lat.beam, G, plan.p.h, plan.p.c, plan.p.ctx_prev,
                                            plan.p.ctx_word, 0), "jlm_seed_context")

    def alt_frames(self, model, plan, rank, sent_off, sent_rows, depth, alt, h0, c0, h1, c1, T, Tm, ld_tm, part, max_parts, rows, prev0,
                   word, target, n_live, n_live_host, nll_seq, nll_tok, flags, n_rows, n_steps, timed):
        import torch
        from jlm_amd import _lib
        o, m = self._o, model.m
        R, S = int(n_rows), int(n_steps)
        assert plan.p.kind == 0 and plan.lat.n_frames >= 1 and 0 <= rank < plan.lat.beam
        assert len(n_live_host) == S and all(0 <= x <= R for x in n_live_host)
        assert word.numel() >= S * R and target.numel() >= S * R and nll_seq.numel() >= R and prev0.numel() >= R
        assert sent_off.numel() >= plan.lat.n_sent + 1 and min(sent_rows.numel(), depth.numel(), alt.numel()) >= R
        p = _lib.ScorePlan()
        p.n_rows, p.n_steps = R, S
        p.h[0], p.h[1], p.c[0], p.c[1], p.T = o(h0), o(h1), o(c0), o(c1), o(T)
        p.Tm, p.ld_tm, p.part, p.max_parts = o(Tm), int(ld_tm), o(part), int(max_parts)
        p.rows, p.prev0, p.word, p.target, p.n_live = o(rows), o(prev0), o(word) if S else None, o(target) if S else None, o(n_live) if S else None
        live = (ctypes.c_int * max(S, 1))(*[int(x) for x in n_live_host])
        p.n_live_host = ctypes.cast(live, ctypes.POINTER(ctypes.c_int))
        p.nll_seq, p.nll_tok, p.flags = o(nll_seq), o(nll_tok), o(flags)
        a = _lib.AltPlan()
        a.n_sent, a.beam, a.n_frames, a.rank = plan.lat.n_sent, plan.lat.beam, plan.lat.n_frames, int(rank)
        a.h, a.c, a.T, a.score, a.lse, a.bp = plan.p.h, plan.p.c, plan.p.T, plan.st.score, plan.st.lse, plan.st.bp
        a.sent_len, a.sent_off, a.sent_rows, a.depth, a.alt, a.prev0 = plan.lat.sent_len, o(sent_off), o(sent_rows), o(depth), o(alt), o(prev0)
        self._chk(self.lib.jlm_alt_frames(m, a, p, 0, None), "jlm_alt_frames")
        return torch.full((S, 4), 1e-3, dtype=torch.float64) if timed and R > 0 else torch.empty(0, dtype=torch.float64)


def install(monkeypatch):
    """fake_hip.install with the doubles above"""
    import torch
    from jlm_amd import _lib, ops

    fake = AltLib()
    monkeypatch.setattr(_lib, "lib", lambda: fake)
    monkeypatch.setattr(_lib, "require_gpu", lambda: torch.device("cpu"))
    monkeypatch.setattr(ops, "_backend", AltOps(fake))
    return fake
