"""What the row-set drivers share: :class:`jlm_amd.score.Scorer`, :class:`jlm_amd.rank.Ranker`, :class:`jlm_amd.generate.Generator`,
:class:`jlm_amd.complete.Completer` and :class:`jlm_amd.context.Primer`.

Each of them is ONE device op over "row sets": two ping-pong sets of LSTM state rows, stepped frame by frame inside the op
(csrc/jlm_decode.hip).  Here: the id and prompt checks made before any launch, the plan of right-aligned prompts that generate and
complete share, the per-call row budget, the buffers every call allocates, and what the teacher-forced calls -- score, rank and their
cached forms -- share besides: the argument check of the stream entry points (:func:`check_streams`) and the setup of a call
(:func:`forced_rows`).  The sentence-mode loop of those calls is :func:`jlm_amd.score.sentence_loop`, their ring
:class:`jlm_amd.cache.Ring`.
"""
import numpy as np

from . import _lib


def check_ids(arr, V, what):
    """ValueError unless every id of ``arr`` lies in [0, V) -- before anything is launched (the kernels index with them)."""
    a = np.asarray(arr)
    if a.size and (a.min() < 0 or a.max() >= V):
        bad = a[(a < 0) | (a >= V)].ravel()[0]
        raise ValueError("%s: word id %d outside the model's vocabulary [0, %d)" % (what, int(bad), V))


def is_int(x):
    return not isinstance(x, bool) and isinstance(x, (int, np.integer))


def check_prompts(prompts, V, what, why):
    """ValueError for an empty prompt (``why`` says what a prompt needs) or an id outside [0, V).  -> prompts as int64 arrays"""
    out = []
    for i, p in enumerate(prompts):
        a = np.asarray(p, dtype=np.int64).ravel()
        if a.size == 0:
            raise ValueError("prompt %d is empty (%s; the reference starts at <eos>)" % (i, why))
        check_ids(a, V, "%s (prompt %d)" % (what, i))
        out.append(a)
    return out


def plan_prompts(lengths, max_rows, rows_per_prompt=1):
    """Prompts sorted by length, longest first (stable), cut into chunks of at most max(1, max_rows // rows_per_prompt) prompts: a
    prompt's rows never split across calls.  Prompts are right-aligned, so the prompts a prompt frame steps are a prefix and all of
    them are live at the last.  -> list of dict(idx = the caller's prompt of each chunk prompt, lens, n_prompt = the longest,
    n_live [n_prompt] = prompts a prompt frame steps)."""
    if max_rows < 1:
        raise ValueError("max_rows must be >= 1")
    per = max(1, int(max_rows) // int(rows_per_prompt))
    lens = np.asarray(lengths, dtype=np.int64)
    order = np.argsort(-lens, kind="stable")
    chunks = []
    for i in range(0, len(order), per):
        idx = order[i:i + per]
        L = lens[idx]
        chunks.append(dict(idx=idx, lens=L, n_prompt=int(L[0]), n_live=live_counts(L)))
    return chunks


def live_counts(lens):
    """n_live [P] int32 of right-aligned prompts of lengths ``lens`` (longest first, P = lens[0]): the prompts frame f steps, those
    with P - f words or more"""
    L = np.asarray(lens, dtype=np.int64)
    P = int(L[0])
    return (L[None, :] >= P - np.arange(P)[:, None]).sum(axis=1).astype(np.int32)


def prompt_arrays(prompts, n_prompt):
    """prompt / prev [n_prompt, R] int32 of right-aligned prompts (longest first): row r consumes its prompt at frames
    n_prompt - len .. n_prompt - 1 and starts from the zero state (prev -1) at the first of them; elsewhere prev = r.  Positions
    before a row's start hold word 0 and prev -1 (never read: the row is not live there)."""
    R = len(prompts)
    prompt = np.zeros((n_prompt, R), dtype=np.int32)
    prev = np.tile(np.arange(R, dtype=np.int32), (n_prompt, 1))
    for r, p in enumerate(prompts):
        f0 = n_prompt - len(p)
        prompt[f0:, r] = p
        prev[:f0 + 1, r] = -1
    return prompt, prev


def clamp_rows(max_rows, budget_bytes, row_bytes, H):
    """rows per call: ``max_rows``, fewer when the call's buffers (``row_bytes`` a row) would exceed ``budget_bytes``, and within the
    LSTM-step kernels' addressing (rows x H / 4 < 2^31)"""
    return int(max(1, min(max_rows, budget_bytes // row_bytes, (0x7ffffff0 // max(H // 4, 1)) - 1)))


def ld_logits(V):
    """the row stride of a call's logits [R, ld_logits] f32: V rounded up to a multiple of 4 (include/jlm_hip.h)"""
    return (V + 3) // 4 * 4


def t_is_state(m):
    """An untied f32 model's T is the state row set the LSTM step wrote, and a call has no T rows of its own.  Every other model
    has them (an untied split-row model: the f32 copy of the state the step writes beside the split rows)."""
    return m.mode == "untied" and not m.split_lstm


class RowSets:
    """The buffers every row-set call allocates, on the device of a :class:`jlm_amd.model.DeviceModel` (inside its context): the
    state row sets h / c, two of [R, H] f32 each, ping-pong; T [R, ldt] f32, None where T is the state (:func:`t_is_state`);
    ``logits`` [R, ld_logits] f32 when asked for; rows = arange(R) int32; the op's flag word, one int32."""

    def __init__(self, m, R, logits=False):
        torch, dev, f32 = m.torch, m.device, m.torch.float32
        e = lambda shape: torch.empty(shape, device=dev, dtype=f32)
        self.h = [e((R, m.H)), e((R, m.H))]
        self.c = [e((R, m.H)), e((R, m.H))]
        self.T = None if t_is_state(m) else e((R, m.ldt))
        self.ld_logits = ld_logits(m.V)
        self.logits = e((R, self.ld_logits)) if logits else None
        self.rows = torch.arange(R, device=dev, dtype=torch.int32)
        self.flags = torch.zeros(1, device=dev, dtype=torch.int32)

    def state(self):
        """the ops' state arguments: h0, c0, h1, c1, T"""
        return self.h[0], self.c[0], self.h[1], self.c[1], self.T

    def after(self, S):
        """(h, c) as a call of S steps leaves them: the row set its last step wrote"""
        return self.h[S % 2], self.c[S % 2]

    def check_flags(self, message, bit0=None):
        """The flag word read back.  JlmHipError(``bit0``) when bit 0 is set and ``bit0`` is given, else JlmHipError(``message`` %
        flags) when any bit is."""
        fl = int(self.flags.cpu()[0])
        if fl & 1 and bit0:
            raise _lib.JlmHipError(bit0)
        if fl:
            raise _lib.JlmHipError(message % fl)


def check_streams(m, inputs, targets, h, c, what=None):
    """The arguments of a stream entry point: ValueError unless inputs / targets are [B, n] arrays of one shape and (h, c) are both None
    or both [B, H].  ``what`` ("score" / "rank"): the ids are checked here, under that label, by a caller that allocates before its
    call's setup (:func:`forced_rows`) checks them.  -> x, y, B, n"""
    x = np.asarray(inputs)
    y = np.asarray(targets)
    if x.ndim != 2 or x.shape != y.shape:
        raise ValueError("inputs and targets must be [B, n] arrays of the same shape (got %s, %s)" % (x.shape, y.shape))
    if (h is None) != (c is None):
        raise ValueError("carry both h and c, or neither")
    B, n = x.shape
    if what:
        check_ids(x, m.V, what)
        check_ids(y, m.V, what)
    check_carried(m, h, c, B)
    return x, y, B, n


def check_carried(m, h, c, R):
    if h is not None and (tuple(h.shape) != (R, m.H) or tuple(c.shape) != (R, m.H)):
        raise ValueError("the carried state must be [%d, %d] (got %s, %s)" % (R, m.H, tuple(h.shape), tuple(c.shape)))


def forced_rows(m, rs, word, target, n_live, h, c, what):
    """The setup of a teacher-forced call, inside the model's context, on the call's :class:`RowSets` ``rs``: word / target [S, R]
    (host) checked and uploaded with n_live, and the carried (h, c) copied into row set 0 (None: the zero state, prev0 = -1).
    -> (S, R, the ops' argument run rows, prev0, word, target, n_live, its host copy)"""
    torch = m.torch
    word = np.ascontiguousarray(word, dtype=np.int32)
    target = np.ascontiguousarray(target, dtype=np.int32)
    S, R = target.shape
    check_ids(word, m.V, what)
    check_ids(target, m.V, what)
    n_live = [int(x) for x in n_live]
    if h is None:
        prev0 = torch.full((R,), -1, device=m.device, dtype=torch.int32)
    else:
        check_carried(m, h, c, R)
        rs.h[0].copy_(h)
        rs.c[0].copy_(c)
        prev0 = rs.rows
    up = lambda a: torch.from_numpy(a).to(m.device)
    return S, R, (rs.rows, prev0, up(word), up(target), up(np.asarray(n_live, dtype=np.int32)), n_live)
