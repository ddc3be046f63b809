"""The error budget of a teacher-forced scoring step, stage by stage (tests/test_gpu_score_budget.py on the device,
tests/test_score_budget_cpu.py on a stand-in).

A scoring step is four launches: the LSTM step, the T projection, the vocabulary normaliser and score_fold_kernel's target logit
(csrc/jlm_decode.hip jlm_score_frames).  Every kernel bar of the suite is a per-launch absolute tolerance; none of them sees the SIGN
of an error or what one stage's error becomes twenty steps later.  Here the difference between the device's per-token -log p and the
float64 oracle's (oracle/jlm_oracle.py OracleLM) is split, exactly, into what each stage adds.  Four trajectories over the same words:

  O     the oracle from the zero state:                                    nll_O(t)
  D     the device, one step per call, its state D_t read back every step: nll_D(t)
  O|D   ONE oracle step from the device's previous state D_{t-1}:          h*_t, nll_OD(t)
  P     the oracle's projection of the device's own hidden state D_t.h:    nll_P(t)

  drift(t) = nll_OD - nll_O        the state error accumulated before step t, propagated in exact arithmetic
  gate(t)  = nll_P  - nll_OD       this step's LSTM-step error
  out(t)   = nll_D  - nll_P        this step's T projection, normaliser and target logit, split with the device's T taken as float64:
    tproj(t) = nll(T_D) - nll_P      nll(T) = lse(T.B^T + b2) - (T.B_w + b2[w]) in float64
    norm(t)  = lse_D - lse(T_D)      lse_D = nll_D + y_D (score_fold_kernel: nll = lse - (double)y)
    logit(t) = y(T_D) - y_D          y_D: the device's f32 target logit (jlm_score_fold, self_norm = 1, on the same T)

and drift + gate + tproj + norm + logit = nll_D - nll_O, term by term.

The same local stages through the numpy restatements of tests/fake_hip.py -- which hold the operand FORMATS (split rows, mixed rows,
the f32 roundings between launches) but accumulate in float64 -- on host copies of the device's stage inputs: a restatement's error
against the oracle is what the formats cost, the device's minus the restatement's what the arithmetic costs (accumulation order, the
hardware exp2 / rcp of the gates, expf in the fold).

Errors of a local stage should be independent from token to token; `unbiased` is the test of that: |mean| <= 4 rms / sqrt(N).  A
common-mode relative error d of h moves a token's nll by (E_p[y_T] - y_T(target)) d, the same sign on nearly every token: it sums over a
sentence like N, not sqrt(N), and fails the test in `gate` at d = 2^-24 (tests/test_score_budget_cpu.py plants it).
"""
import numpy as np

STAGES = ("drift", "gate", "tproj", "norm", "logit")
LOCAL = STAGES[1:]
U = 2.0 ** -24
CHUNK = 256                    # rows per float64 logit block [CHUNK, V]


def lse(y):
    m = y.max(axis=-1, keepdims=True)
    return (m + np.log(np.exp(y - m).sum(axis=-1, keepdims=True)))[..., 0]


def _pad4(n):
    return (n + 3) // 4 * 4


# ------------------------------------------------------------------------------------------------ the oracle's T, in the device's layout
def t_layout(lm):
    """([(t_off, size) per segment], ldt) of a T row as jlm_amd/model.py DeviceModel lays it out: tied [h.PM]; D-softmax the same
    product with every segment's columns at a 4-aligned offset; D-softmax* [h.PM | (h.PM).VT1^T | ...]"""
    assert lm.share_embedding, "an untied model's T is the state itself"
    if not (lm.config["D_softmax"] or lm.config["V_table"]):
        E = lm.weights["PM"].shape[1]
        return [(0, E)], _pad4(E)
    offs, off = [], 0
    for size, _s, _e in lm.segs:
        offs.append((off, size))
        off += _pad4(size)
    return offs, off


def oracle_T(lm, h):
    """T of hidden states h [N, H] in float64, the reference's own products (decoder/model.py:145-186), in t_layout's columns"""
    offs, ldt = t_layout(lm)
    t = np.dot(h, lm.weights["PM"])
    T = np.zeros((len(h), ldt))
    if lm.config["V_table"]:
        for i, (off, size) in enumerate(offs):
            T[:, off:off + size] = t if i == 0 else np.dot(t, lm.v_tables[i].T)
    elif lm.config["D_softmax"]:
        c0 = 0
        for off, size in offs:
            T[:, off:off + size] = t[:, c0:c0 + size]
            c0 += size
    else:
        T[:, :t.shape[1]] = t
    return T


def _blocks(lm):
    return lm.blocks if lm.blocks is not None else [lm.weights["LM"]]


def logits_from_T(lm, T):
    """the oracle's logits [N, V] of T rows given as float64 (f32 weights meet float64 operands, as in OracleLM.project)"""
    offs, _ldt = t_layout(lm)
    ys = [np.dot(T[:, off:off + size], blk.T) for (off, size), blk in zip(offs, _blocks(lm))]
    return np.concatenate(ys, axis=1) + lm.weights["b2"]


def lse_and_target(logits_of, X, tgt):
    """(log-normaliser, target logit) [N] of the rows X under `logits_of`, a block of CHUNK rows at a time"""
    N = len(tgt)
    l, y = np.empty(N), np.empty(N)
    for a in range(0, N, CHUNK):
        Y = logits_of(X[a:a + CHUNK])
        l[a:a + CHUNK] = lse(Y)
        y[a:a + CHUNK] = Y[np.arange(len(Y)), tgt[a:a + CHUNK]]
    return l, y


def logit_bound(lm, T, tgt):
    """Worst-case rounding bound of score_fold_kernel's target logit on these operands: n u / (1 - n u) (sum_k |T_k B_wk| + |b2[w]|).
    Its documented chain (csrc/jlm_score.hip): lane `sub` of eight takes the 16-byte chunks sub, sub + 8, ... and runs fmaf in k order
    -- 4 ceil(ceil(k / 4) / 8) roundings on the longest lane --, three pairwise adds, + b2[w]: n = that + 4."""
    offs, _ldt = t_layout(lm)
    out = np.empty(len(tgt))
    v0 = 0
    for (off, size), blk in zip(offs, _blocks(lm)):
        sel = np.nonzero((tgt >= v0) & (tgt < v0 + blk.shape[0]))[0]
        n = 4 * -(-_pad4(size) // 4 // 8) + 4
        mag = np.abs(T[sel, off:off + size] * blk[tgt[sel] - v0].astype(np.float64)).sum(axis=1) + np.abs(lm.weights["b2"][tgt[sel]])
        out[sel] = n * U / (1.0 - n * U) * mag
        v0 += blk.shape[0]
    return out


# ------------------------------------------------------------------------------------------------ the record of a stepped run
class Steps:
    """What a device (or a stand-in) reports of R rows stepped S times, one step per call.  x, y [R, S] the words consumed and scored
    on; lens [R] (steps past a row's length are ignored); nll [S, R] the per-token -log p; h, c [S, R, H] the state after every step
    as float64 values; T [S, R, ldt] the step's T rows as float64; ylog [S, R] the device's own target logit."""

    def __init__(self, x, y, lens, nll, h, c, T, ylog):
        self.x, self.y, self.lens = np.asarray(x), np.asarray(y), np.asarray(lens)
        self.nll, self.h, self.c, self.T, self.ylog = nll, h, c, T, ylog


def sentence_steps(seqs, start):
    """x, y [R, S], lens of ragged sentences stepped as LSTM_Model.score steps them; padding consumes and scores word `start`"""
    lens = np.array([len(s) for s in seqs])
    R, S = len(seqs), int(lens.max())
    x = np.full((R, S), start, dtype=np.int64)
    y = np.full((R, S), start, dtype=np.int64)
    for r, s in enumerate(seqs):
        y[r, :len(s)] = s
        x[r, 1:len(s)] = s[:-1]
    return x, y, lens


def chosen_sentences(lm, start, lens, choose):
    """sentences whose every next word is choose(the oracle's logits, axis = 1) -- np.argmax: the words a model finds likely, the regime
    of real text; row r starts from word start[r] and the zero state -> word-id lists of lengths lens"""
    R = len(lens)
    h, c = lm.zero_state(R)
    word = np.asarray(start, dtype=np.int64).copy()
    out = np.empty((R, int(max(lens))), dtype=np.int64)
    for t in range(out.shape[1]):
        h, c = lm.lstm_cell(word, h, c)
        word = choose(lm.project(h), axis=1)
        out[:, t] = word
    return [list(out[r, :L]) for r, L in enumerate(lens)]


class Budget:
    """The stage terms of every live token, flat ([N], step-major): `dev` and `fmt` {stage: [N]} (fmt: the restatements', local
    stages only, None without them), total = nll_D - nll_O, step / row [N] of each token, bound = logit_bound."""

    def __init__(self, step, row, dev, fmt, total, bound, nll_d, nll_o, lse_d=None, gate_ulp=None):
        self.step, self.row, self.dev, self.fmt, self.total, self.bound, self.nll_d, self.nll_o = step, row, dev, fmt, total, bound, nll_d, nll_o
        self.lse_d, self.gate_ulp = lse_d, gate_ulp
        self.n_rows = int(row.max()) + 1

    def half_ulp_caps(self):
        """What a same-signed error of half an f32 ulp of a stage's own output would be, per token: of the hidden state -- h (1 + 2^-24),
        through the oracle's projection -- for gate, of the log-normaliser for norm.  A stage whose errors share a sign is held under
        this: its bias is then below the precision of the number format its result is stored in."""
        return dict(gate=abs(float(self.gate_ulp.mean())), norm=U * float(np.maximum(1.0, np.abs(self.lse_d)).mean()))

    def sentence_sums(self, e):
        return np.bincount(self.row, weights=e, minlength=self.n_rows)


def oracle_run(lm, x):
    """the oracle from the zero state over x [R, S] -> h [S, R, H]"""
    R, S = x.shape
    h, c = lm.zero_state(R)
    out = np.empty((S, R, lm.hidden_size))
    for t in range(S):
        h, c = lm.lstm_cell(x[:, t], h, c)
        out[t] = h
    return out


def decompose(lm, st, restated=None):
    """-> Budget.  restated: dict(h [S, R, H] the restated LSTM step from D_{t-1}, T [S, R, ldt] the restated T projection of D_t.h,
    lse [S, R] the restated normaliser of the device's T, ylog [S, R] the restated target logit of the device's T), or None.
    Asserts the two identities: the stage terms sum to nll_D - nll_O within 1e-12, and lse_D - y_D gives nll_D back to one f64 ulp."""
    assert not lm.config["self_norm"]
    R, S = st.x.shape
    live = np.arange(S)[:, None] < st.lens[None, :]                       # [S, R]
    ti, ri = np.nonzero(live)
    tgt = st.y[ri, ti]
    project = lambda X: lm.project(X)
    from_T = lambda X: logits_from_T(lm, X)
    nll_of = lambda f, X: np.subtract(*lse_and_target(f, X, tgt))
    # O
    nll_o = nll_of(project, oracle_run(lm, st.x)[ti, ri])
    # O|D: one oracle step from D_{t-1} (the zero state before step 0)
    zero = np.zeros((1, R, lm.hidden_size))
    h_prev, c_prev = np.concatenate([zero, st.h[:-1]])[ti, ri], np.concatenate([zero, st.c[:-1]])[ti, ri]
    h_star, _c = lm.lstm_cell(st.x[ri, ti], h_prev, c_prev)
    nll_od = nll_of(project, h_star)
    # P, and the device's T as float64
    nll_p = nll_of(project, st.h[ti, ri])
    T_d = st.T[ti, ri]
    lse_t, y_t = lse_and_target(from_T, T_d, tgt)
    nll_d, y_d = st.nll[ti, ri], st.ylog[ti, ri]
    lse_d = nll_d + y_d
    assert (np.abs((lse_d - y_d) - nll_d) <= np.spacing(np.abs(nll_d))).all(), "lse_D - y_D does not give the step's nll back"
    dev = dict(drift=nll_od - nll_o, gate=nll_p - nll_od, tproj=(lse_t - y_t) - nll_p, norm=lse_d - lse_t, logit=y_t - y_d)
    total = nll_d - nll_o
    gap = np.abs(sum(dev[s] for s in STAGES) - total).max()
    assert gap <= 1e-12, ("the five stages do not sum to nll_D - nll_O", gap)
    out = nll_d - nll_p
    assert np.abs(dev["tproj"] + dev["norm"] + dev["logit"] - out).max() <= 1e-12
    fmt = None
    if restated is not None:
        lse_tr, y_tr = lse_and_target(from_T, restated["T"][ti, ri], tgt)
        fmt = dict(gate=nll_of(project, restated["h"][ti, ri]) - nll_od, tproj=(lse_tr - y_tr) - nll_p,
                   norm=restated["lse"][ti, ri] - lse_t, logit=y_t - restated["ylog"][ti, ri])
    gate_ulp = nll_of(project, st.h[ti, ri] * (1.0 + U)) - nll_p
    return Budget(ti, ri, dev, fmt, total, logit_bound(lm, T_d, tgt), nll_d, nll_o, lse_d, gate_ulp)


# ------------------------------------------------------------------------------------------------ figures
def unbiased(e):
    """errors of different tokens independent: |mean| <= 4 rms / sqrt(N) -> (ok, mean, bar)"""
    e = np.asarray(e, dtype=np.float64)
    rms = float(np.sqrt(np.mean(e * e)))
    bar = 4.0 * rms / np.sqrt(len(e))
    return abs(float(e.mean())) <= bar, float(e.mean()), bar


def figures(b, e):
    """(mean, rms, max |.| over tokens; max |.| and rms of the per-sentence sums)"""
    s = b.sentence_sums(e)
    return (float(e.mean()), float(np.sqrt(np.mean(e * e))), float(np.abs(e).max()), float(np.abs(s).max()),
            float(np.sqrt(np.mean(s * s))))


def table(title, b):
    """one table: per stage the device's figures, beside them the restatement's (format cost) and device - restatement (arithmetic)"""
    rows = ["%s: %d tokens, %d sentences" % (title, len(b.total), b.n_rows),
            "  %-6s %-6s %10s %10s %10s | %10s %10s | 4rms/sqrtN" % ("stage", "", "mean", "rms", "max", "sent max", "sent rms")]
    fmt = lambda f: " ".join("%10.2e" % v for v in f[:3]) + " | " + " ".join("%10.2e" % v for v in f[3:])
    for s in STAGES:
        ok, _mean, bar = unbiased(b.dev[s])
        rows.append("  %-6s %-6s %s | %8.2e %s" % (s, "device", fmt(figures(b, b.dev[s])), bar,
                                                    "" if s == "drift" else "unbiased" if ok else "BIASED"))
        if b.fmt is not None and s in b.fmt:
            rows.append("  %-6s %-6s %s |" % ("", "format", fmt(figures(b, b.fmt[s]))))
            rows.append("  %-6s %-6s %s |" % ("", "arith", fmt(figures(b, b.dev[s] - b.fmt[s]))))
    rows.append("  %-6s %-6s %s |" % ("sum", "device", fmt(figures(b, sum(b.dev[s] for s in STAGES)))))
    rows.append("  %-6s %-6s %s |" % ("total", "device", fmt(figures(b, b.total))))
    if b.gate_ulp is not None:
        caps = b.half_ulp_caps()
        rows.append("  a same-signed half ulp of f32: of h %.2e per token (gate), of the log-normaliser %.2e (norm)" % (caps["gate"], caps["norm"]))
    return "\n".join(rows)


# ------------------------------------------------------------------------------------------------ the restatements, on host copies
def host_model(m, words):
    """tests/fake_hip.py _FakeModel over host copies of a jlm_amd.model.DeviceModel's own operands, assembled as
    DeviceModel.decode_model assembles them; of the gate table xgate8 [V, 4H] the rows of `words` only (-> model, words as table rows)"""
    from tests.fake_hip import _FakeModel
    cpu = lambda t: t.detach().cpu().contiguous()
    uniq, inv = np.unique(np.asarray(words).ravel(), return_inverse=True)
    t = dict(b2=cpu(m.b2), wt8=cpu(m.wt8), pmt_split=cpu(m.pmt_split),
             xgate8=cpu(m.xgate8[m.torch.as_tensor(uniq, device=m.xgate8.device)]))
    rows = m.mixed
    if rows is not None and rows.b2_log2 is not None:
        t["b2_log2"] = cpu(rows.b2_log2)
    i = dict(H=m.H, ldt=m.ldt, untied=0, self_norm=0, split_lstm=1, n_t=m.pmt.shape[0])
    f = dict(gate_descale=m.gate_descale, h_scale=m.h_scale, t_descale=m.t_descale)
    meta = lambda segs: [int(sg[k]) for sg in segs for k in ("v_start", "v_end", "k", "t_off", "ldb")]
    sp = ([cpu(b) for b in m.seg_split], meta(m.split_segments), [float(v) for v in m.split_t_scale],
          [float(v) for v in m.split_descale], [int(v) for v in m.split_bias_col])
    mx = ([], [], [], [], [], [], [])
    if rows is not None:
        mx = (rows.idx, [cpu(s.packed) for s in rows.segs], meta(s.seg for s in rows.segs), [float(s.t_scale) for s in rows.segs],
              [float(s.descale) for s in rows.segs], [float(s.s8) for s in rows.segs], [int(v) for v in rows.head_split])
    return _FakeModel(t, i, f, [cpu(b) for b in m.seg_B], meta(m.segments), *(sp + mx)), inv.reshape(np.shape(words))


def _restated_lse(FK, fm, T, ld_tm):
    """the normaliser of the host T rows [n, ldt] f32 in the form csrc/jlm_decode.hip full_lse_pack / full_lse_run launch it for this
    model (mixed rows, the hybrid launch, split rows), its slices folded in float64 -> lse [n]"""
    import torch
    from jlm_amd import _lib
    m = fm.m
    n = T.shape[0]
    ptr = lambda a: a.data_ptr()
    part = torch.zeros((96, n, 2), dtype=torch.float32)
    r = -2
    if m.mixed_segs and ld_tm:
        idx = [i for i in range(m.n_segs) if m.mixed_segs[i].B]
        only = (_lib.Segment * len(idx))(*[m.mixed_segs[i] for i in idx])
        assert FK.jlm_mixed_t_stride(only, len(idx)) == ld_tm
        Tm = torch.zeros(((n + 31) // 32 * 32, ld_tm), dtype=torch.float32)
        assert FK._pack_t_for(m)(only, [m.mixed_t_scale[i] for i in idx], len(idx), ptr(T), m.ldt, None, n, None, ptr(Tm), ld_tm, 0) == 0
        cut = bool(m.mixed_head_split) and any(m.mixed_head_split[i] > 0 for i in idx)
        if len(idx) == m.n_segs and not cut:
            r = FK.jlm_vocab_lse_mixed(m.mixed_segs, m.mixed_descale, m.mixed_s8, m.mixed_bias2, m.n_segs, ptr(Tm), ld_tm, ptr(part), n, 96,
                                       n, None, 0)
        else:
            r = FK.jlm_vocab_lse_hybrid(m.split_segs, m.split_t_scale, m.split_descale, m.split_bias_col, m.mixed_segs, m.mixed_descale,
                                        m.mixed_s8, m.mixed_head_split, m.n_segs, m.b2, ptr(T), m.ldt, ptr(Tm), ld_tm, None, ptr(part), n,
                                        96, n, None, 0)
    if r == -2:
        r = FK.jlm_vocab_lse_split(m.split_segs, m.split_t_scale, m.split_descale, m.split_bias_col, m.n_segs, m.b2, ptr(T), m.ldt, None,
                                   ptr(part), n, 96, n, None, 0)
    assert r >= 1, r
    p = part[:r].numpy().astype(np.float64)
    mx = p[:, :, 0].max(axis=0)
    return mx + np.log((p[:, :, 1] * np.exp(p[:, :, 0] - mx)).sum(axis=0))


def restate(m, x, y, h_raw, c_raw, T_raw):
    """The gate, tproj, norm and logit stages of a split-row DeviceModel through FakeLib, on host copies of the device's stage inputs:
    h_raw [S, R, H] the state rows as the device holds them (split rows in f32-typed storage), c_raw [S, R, H] f32, T_raw [S, R, ldt]
    f32 (host torch tensors).  -> the `restated` dict of decompose()."""
    import torch
    from tests.fake_hip import FakeLib
    FK = FakeLib()
    S, R, H = h_raw.shape
    N = S * R
    fm, wrow = host_model(m, x.T)                                         # [S, R] table rows
    ptr = lambda a: a.data_ptr()
    # the LSTM step of every (t, r) from D_{t-1}: rows N .. 2N - 1 step from rows 0 .. N - 1, the rows of step 0 from the zero state
    h_io, c_io = torch.zeros((2 * N, H), dtype=torch.float32), torch.zeros((2 * N, H), dtype=torch.float32)
    h_io[R:N], c_io[R:N] = h_raw[:-1].reshape(-1, H), c_raw[:-1].reshape(-1, H)
    rows = torch.arange(N, 2 * N, dtype=torch.int32)
    prev = torch.arange(-N, N, dtype=torch.int32)
    prev[N:N + R] = -1
    word = torch.zeros(2 * N, dtype=torch.int32)
    word[N:] = torch.as_tensor(wrow.reshape(-1), dtype=torch.int32)
    assert FK.jlm_lstm_step_xg(ptr(h_io), ptr(c_io), H, ptr(h_io), ptr(c_io), ptr(rows), ptr(prev), ptr(word), fm.m.wt8, fm.m.xgate8, H,
                               fm.m.gate_descale, fm.m.h_scale, None, N, None, 0) == 0
    h_r = FK._split_read(ptr(h_io), 2 * N, H)[N:] / fm.m.h_scale
    # the T projection of D_t.h
    A = h_raw.reshape(N, H).contiguous()
    T_r = torch.zeros((N, m.ldt), dtype=torch.float32)
    assert FK.jlm_gemm_nt_split(ptr(A), H, None, fm.m.pmt_split, H, None, ptr(T_r), m.ldt, None, None, fm.m.t_descale, N, fm.m.n_t, H, None,
                                0) == 0
    # the normaliser and the target logit of the device's T
    T_d = T_raw.reshape(N, m.ldt).contiguous()
    lse_r = np.concatenate([_restated_lse(FK, fm, T_d[a:a + CHUNK].contiguous(), int(m.ld_tm or 0)) for a in range(0, N, CHUNK)])
    tgt = torch.as_tensor(np.ascontiguousarray(y.T).reshape(-1), dtype=torch.int32)
    seq, tok = torch.zeros(N, dtype=torch.float64), torch.zeros(N, dtype=torch.float64)
    assert FK.jlm_score_fold(fm.m.segs, fm.m.n_segs, fm.m.b2, ptr(T_d), m.ldt, None, N, 0, 1, ptr(tgt), None, N, ptr(seq), ptr(tok), None,
                             0) == 0
    return dict(h=h_r.reshape(S, R, H), T=T_r.numpy().astype(np.float64).reshape(S, R, m.ldt), lse=lse_r.reshape(S, R),
                ylog=-tok.numpy().reshape(S, R))


# ------------------------------------------------------------------------------------------------ a stand-in device
def stand_in_steps(lm, x, y, lens, h_bias=0.0, round_T=False):
    """The oracle as a "device": its state rounded to f32 after every step, its log-normaliser and target logit rounded to f32 as
    score_fold_kernel holds them.  Plants: h_bias -- h (1 + h_bias) after every step, a common-mode relative error of the hidden
    state; round_T -- T rounded to f32."""
    R, S = x.shape
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    h, c = lm.zero_state(R)
    hs, cs, Ts = np.empty((S, R, lm.hidden_size)), np.empty((S, R, lm.hidden_size)), []
    nll, ylog = np.empty((S, R)), np.empty((S, R))
    for t in range(S):
        h, c = lm.lstm_cell(x[:, t], h, c)
        h, c = f32(h) * (1.0 + h_bias), f32(c)
        T = oracle_T(lm, h)
        T = f32(T) if round_T else T
        Y = logits_from_T(lm, T)
        yt = f32(Y[np.arange(R), y[:, t]])
        hs[t], cs[t], ylog[t], nll[t] = h, c, yt, f32(lse(Y)) - yt
        Ts.append(T)
    return Steps(x, y, lens, nll, hs, cs, np.stack(Ts), ylog)
