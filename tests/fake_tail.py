"""The numpy double of ``jlm_tail_predict`` / ``torch.ops.jlm.tail_predict`` for the CPU-only suite: tests/fake_hip.py's FakeLib and
FakeOps with the one entry point more (that file stays as it is).  TEST INFRASTRUCTURE ONLY; it restates the contract written in
include/jlm_hip.h, not the HIP code.
"""
import numpy as np

from tests import fake_hip
from tests.fake_hip import _p, view


class TailLib(fake_hip.FakeLib):
    def jlm_tail_predict(self, segs, n_segs, b2, T, ldt, n_sent, beam, n_frames, score, lse, cnt, bp, node, mode, ids, n_ids, sp_off,
                         sp_frame, sp_lo, sp_hi, n_out, chunk, out_score, out_row, out_word, out_nodes, out_len, stride, stream):
        if not (1 <= n_out <= 64 and 1 <= beam <= 1024 and ldt % 4 == 0 and mode in (0, 1) and chunk >= 0 and stride >= 1):
            return -1
        if not all(_p(x) for x in (b2, T, score, cnt, bp, node, ids, sp_off, sp_frame, sp_lo, sp_hi, out_score, out_row, out_word,
                                   out_nodes, out_len)) or (mode == 0 and not _p(lse)):
            return -1
        if n_sent <= 0:
            return 0
        sg = self._segs(segs, n_segs)
        rmax, G = n_sent * beam, n_frames * n_sent * beam
        sc, cn = view(score, G, np.float64), view(cnt, n_frames * n_sent, np.int32)
        ls = view(lse, G, np.float64) if mode == 0 else None
        bpv, nd = view(bp, G, np.int32), view(node, G, np.int32)
        idv = view(ids, n_ids, np.int32) if n_ids else np.zeros(0, np.int32)
        off = view(sp_off, n_sent + 1, np.int32)
        n_sp = int(off[-1])
        fr, lo, hi = (view(a, n_sp, np.int32) if n_sp else np.zeros(0, np.int32) for a in (sp_frame, sp_lo, sp_hi))
        R = n_sent * n_out
        osc, orow, owd, oln = view(out_score, R, np.float64), view(out_row, R, np.int32), view(out_word, R, np.int32), view(out_len, R, np.int32)
        ond = view(out_nodes, R * stride, np.int32).reshape(R, stride)
        for s in range(n_sent):
            keys, rows, words = [], [], []
            for j in range(int(off[s]), int(off[s + 1])):
                f, a, b = int(fr[j]), int(lo[j]), int(hi[j])
                if not (0 <= f < n_frames and 0 <= a < b <= n_ids):
                    continue
                nrows = min(int(cn[f * n_sent + s]), beam)
                if nrows <= 0:
                    continue
                g0 = f * rmax + s * beam
                y = self._word_logits(sg, b2, T, ldt, g0, nrows, idv[a:b])                  # [words, rows] float32
                base = sc[g0:g0 + nrows] + ls[g0:g0 + nrows] if mode == 0 else sc[g0:g0 + nrows]
                keys.append((base[None, :] - y.astype(np.float64)).reshape(-1))
                rows.append(np.tile(np.arange(g0, g0 + nrows), b - a))
                words.append(np.repeat(idv[a:b], nrows))
            o = s * n_out
            osc[o:o + n_out], orow[o:o + n_out], owd[o:o + n_out], oln[o:o + n_out] = np.inf, -1, -1, 0
            if not keys:
                continue
            keys, rows, words = np.concatenate(keys), np.concatenate(rows), np.concatenate(words)
            order = np.argsort(keys, kind="stable")
            order = order[~np.isnan(keys[order])][:n_out]                                    # a NaN score never ranks
            for r, c in enumerate(order):
                osc[o + r], orow[o + r], owd[o + r] = keys[c], rows[c], words[c]
                g, d = int(rows[c]), 0
                while g >= 0 and d < stride:
                    ond[o + r, d] = nd[g]
                    d += 1
                    g = int(bpv[g])
                oln[o + r] = d
        return 0


class TailOps(fake_hip.FakeOps):
    def __init__(self, lib=None):
        fake_hip.FakeOps.__init__(self, lib or TailLib())

    def tail_predict(self, model, plan, ids, sp_off, sp_frame, sp_lo, sp_hi, n_out, chunk, out_score, out_row, out_word, out_nodes, out_len,
                     stride):
        m, o = model.m, self._o
        assert plan.p.kind != 2 and plan.lat.n_frames >= 1
        self._chk(self.lib.jlm_tail_predict(m.segs, m.n_segs, m.b2, plan.p.T, m.ldt, plan.lat.n_sent, plan.lat.beam, plan.lat.n_frames,
                                            plan.st.score, plan.st.lse, plan.st.cnt, plan.st.bp, plan.st.node, 1 if m.self_norm else 0,
                                            o(ids), int(ids.numel()), o(sp_off), o(sp_frame), o(sp_lo), o(sp_hi), int(n_out), int(chunk),
                                            o(out_score), o(out_row), o(out_word), o(out_nodes), o(out_len), int(stride), 0),
                  "jlm_tail_predict")


def install(monkeypatch):
    """fake_hip.install with the doubles above"""
    import torch
    from jlm_amd import _lib, ops

    fake = TailLib()
    monkeypatch.setattr(_lib, "lib", lambda: fake)
    monkeypatch.setattr(_lib, "require_gpu", lambda: torch.device("cpu"))
    monkeypatch.setattr(ops, "_backend", TailOps(fake))
    return fake
