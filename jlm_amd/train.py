"""Training of the LSTM language model on the device: ``train_experiment``, ``python -m jlm_amd.train``.

The reference trains with TensorFlow 1 and sacred (train/model.py ``RNNLM_Model``, train/train.py) and dumps the weights with
train/weights.py.  Here the same graph is trained by the kernels of csrc/jlm_train.hip and the files written are the ones
``jlm_amd.weights.load_weights`` / ``config.load_config_dict`` read: a trained experiment loads into ``LSTM_Model``, ``Decoder``,
``jlm_amd.perplexity`` and ``jlm_amd.compress`` as it is.

The step, with B = batch_size, T = num_steps, N = B T rows in time-major order (row = t B + b):
  Emb [V, E]   tied: ``LM``; V_table: ``LM0`` on top of ``LM{i} VT{i}``, E = embedding_seg[0][0]; D_softmax: the block-diagonal matrix of
               the ``LM`` block list, E = the sum of the widths
  x_t = mask_in (.) Emb[input[:, t]]                      masks in {0, 1 / keep}
  z = h HM + x IM + b, gates i | f | o | g;  c = c f + g i;  h = tanh(c) o;  r_t = mask_out (.) h_t
  P = r PM;  y = P Emb^T + b2;  ce = mean(lse - y[target]);  loss = ce + norm_weight mean(lse^2) with self_norm
  the last h, c are the next chunk's first; no gradient crosses chunks.  Adam in TensorFlow's form, every element every step.

:class:`ReferenceStepper` is that step in numpy float64 with a hand-written backward pass: what :class:`DeviceStepper` is judged against
(tests/test_gpu_train.py), itself pinned to torch autograd (tests/test_train_cpu.py).  Both draw the same dropout masks
(:func:`dropout_mask`: a pure function of seed, step, site and element) and start from the same :func:`init_weights`.

On the device torch allocates, copies and sorts a step's input ids; every contraction is ``jlm_train_gemm`` (an f32 fmaf chain in k
order), every sum has one writer and a fixed order, so the same parameters and corpus write the same bytes run after run.  The vocabulary
loss never holds [N, V]: the logits are computed in chunks of words bounded by ``TRAIN_CHUNK_BYTES``, once for the normaliser and once
more for ``dy``, segment by segment: a D_softmax block meets its columns of P, a V_table segment i > 0 works in the factored form
(``Q_i = P VT_i^T``, ``dLM_i = dy^T Q_i``, ``dQ_i = dy LM_i``, ``dVT_i = dQ_i^T P``, ``dP += dQ_i VT_i``), so the cost stays
sum V_i k_i as in inference.  The input side gathers from a dense Emb assembled before the step and sends its gradient back through
the factorisation (``dLM_i += D VT_i^T``, ``dVT_i += LM_i^T D``), all in a fixed order.

There is no CPU fallback for real training: ``train_experiment`` needs the GPU, like the rest of the package.
"""
import argparse
import json
import math
import os
import pickle
import time

import numpy as np

from . import config as _config
from .compress import mix as _mix

GATES = "ifog"
TRAIN_CHUNK_BYTES = int(os.environ.get("JLM_TRAIN_CHUNK_BYTES", 256 << 20))     # the logits scratch of the vocabulary loss
BETA1, BETA2, EPSILON = 0.9, 0.999, 1e-8
SITE_INPUT, SITE_OUTPUT = 0, 1
_M64 = (1 << 64) - 1
_GOLDEN = 0x9E3779B97F4A7C15

# train/train.py:13-36
DEFAULTS = {
    "debug": False,
    "gpu_id": 1,
    "vocab_size": 100000,
    "optimizer": "adam",
    "batch_size": 128,
    "embed_size": 256,
    "hidden_size": 256,
    "num_steps": 20,
    "max_epochs": 20,
    "early_stopping": 1,
    "dropout": 0.9,
    "lr": 0.001,
    "tf_random_seed": 101,
    "share_embedding": True,
    "D_softmax": False,
    "V_table": False,
    "embedding_seg": [(256, 0, 4000), (128, 4000, 12000), (64, 12000, None)],
    "char_rnn": False,
    "self_norm": True,
    "norm_weight": 0.1,
    "class_based": False,
    "class_size": 200,
}


class NonFiniteLoss(RuntimeError):
    """the loss of a step is not finite; ``epoch`` (set by the driver) and ``step`` say where"""

    def __init__(self, step, epoch=None):
        self.step, self.epoch = int(step), epoch
        RuntimeError.__init__(self, "the loss is not finite at epoch {}, step {}".format(epoch, step))


def check_parameters(parameters):
    """DEFAULTS overlaid with ``parameters``; ValueError / NotImplementedError for what is not built, before any launch."""
    unknown = sorted(set(parameters) - set(DEFAULTS))
    if unknown:
        raise ValueError("unknown training parameters: %s" % ", ".join(unknown))
    p = dict(DEFAULTS)
    p.update(parameters)
    if p["class_based"]:
        raise ValueError("class_based models are not built (the inference side cannot run one either)")
    if p["optimizer"] != "adam":
        raise ValueError("optimizer must be 'adam' (got %r)" % (p["optimizer"],))
    if not p["share_embedding"]:
        raise NotImplementedError("share_embedding=False (an untied projection UM) is not built")
    if p["D_softmax"] and p["V_table"]:
        raise ValueError("D_softmax and V_table exclude each other")
    if not 0.0 < float(p["dropout"]) <= 1.0:
        raise ValueError("dropout is a keep probability in (0, 1]")
    for k in ("batch_size", "num_steps", "hidden_size", "embed_size", "vocab_size"):
        if int(p[k]) < 1:
            raise ValueError("%s must be >= 1" % k)
    p["embedding_seg"] = [list(s) for s in p["embedding_seg"]]
    return p


# ------------------------------------------------------------------------------------------------- shapes, initial weights
def model_dims(cfg, n_out=None):
    """-> dict(kind = tied | vtable | dsoftmax, V, H, E, segs = [(width, start, end)] with the open end resolved)"""
    V = int(cfg["vocab_size"] if n_out is None else n_out)
    segs = []
    for size, s, e in cfg["embedding_seg"]:
        segs.append((int(size), int(s), V if e is None else int(e)))
    if cfg.get("V_table"):
        kind, E = "vtable", segs[0][0]
    elif cfg.get("D_softmax"):
        kind, E = "dsoftmax", sum(s[0] for s in segs)
    else:
        kind, E, segs = "tied", int(cfg["embed_size"]), []
    if segs:
        if segs[0][1] != 0 or segs[-1][2] != V or any(a[2] != b[1] for a, b in zip(segs, segs[1:])) or any(e <= s for _z, s, e in segs):
            raise ValueError("embedding_seg must cut [0, %d) into consecutive non-empty ranges (got %r)" % (V, cfg["embedding_seg"]))
    return dict(kind=kind, V=V, H=int(cfg["hidden_size"]), E=E, segs=segs)


def glorot_limit(shape):
    """tf.get_variable's default initialiser: uniform within sqrt(6 / (fan_in + fan_out)); a 1-D tensor has fan_in = fan_out = n"""
    fan_in, fan_out = (shape[0], shape[0]) if len(shape) == 1 else (shape[0], shape[1])
    return math.sqrt(6.0 / (fan_in + fan_out))


def weight_shapes(cfg, n_out=None):
    """The dump's tensors in the order init_weights draws them: list of (key, block index or None, shape, shape the Glorot limit is
    taken from).  The D_softmax blocks are parts of the reference's one masked [V, E] variable, so they take its limit."""
    d = model_dims(cfg, n_out)
    V, H, E = d["V"], d["H"], d["E"]
    out = [("HM" + g, None, (H, H), (H, H)) for g in GATES]
    out += [("IM" + g, None, (E, H), (E, H)) for g in GATES]
    out += [("b" + g, None, (H,), (H,)) for g in GATES]
    out += [("b2", None, (V,), (V,)), ("PM", None, (H, E), (H, E))]
    if d["kind"] == "vtable":
        for i, (size, s, e) in enumerate(d["segs"]):
            out.append(("LM%d" % i, None, (e - s, size), (e - s, size)))
            if i:
                out.append(("VT%d" % i, None, (size, E), (size, E)))
    elif d["kind"] == "dsoftmax":
        for i, (size, s, e) in enumerate(d["segs"]):
            out.append(("LM", i, (e - s, size), (V, E)))
    else:
        out.append(("LM", None, (V, E), (V, E)))
    return out


def init_weights(cfg, n_out=None, seed=101):
    """Glorot-uniform float32 weights with synth.make_weights' keys and shapes, drawn from numpy.random.RandomState(seed) in
    weight_shapes' order: HM, IM, b (each i, f, o, g), b2, PM, then the embedding tensors."""
    rng = np.random.RandomState(seed)
    w = {}
    for key, idx, shape, fan in weight_shapes(cfg, n_out):
        lim = glorot_limit(fan)
        a = rng.uniform(-lim, lim, size=shape).astype(np.float32)
        if idx is None:
            w[key] = a
        else:
            w.setdefault(key, []).append(a)
    return w


def _items(w):
    """(key, block index or None, array) of every tensor of a dump-shaped dict, in sorted key order"""
    for k in sorted(w):
        if isinstance(w[k], list):
            for i, a in enumerate(w[k]):
                yield k, i, a
        else:
            yield k, None, w[k]


def _map(w, fn):
    return {k: [fn(a) for a in v] if isinstance(v, list) else fn(v) for k, v in w.items()}


# ------------------------------------------------------------------------------------------------- dropout, Adam
def mask_key(seed, step, site):
    """the 64-bit key of one mask: the package's splitmix64 of (seed, step, site)"""
    return _mix(int(seed) & _M64, int(step), int(site))


def keep_threshold(keep):
    """keep <=> a 24-bit uniform integer < ceil(keep 2^24): the host and the device compare integers, not rounded floats"""
    return min(max(int(math.ceil(float(keep) * (1 << 24))), 0), 1 << 24)


def keep_bits(key, start, count, thr):
    """bool [count]: the keep decisions of elements [start, start + count) under ``key``"""
    with np.errstate(over="ignore"):
        z = np.uint64(key) + np.uint64(_GOLDEN) * (np.arange(start, start + count, dtype=np.uint64) + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(40)).astype(np.int64) < thr


def dropout_mask(seed, step, site, shape, keep, offset=0):
    """The mask of tf.nn.dropout as a pure function of its arguments: float64 ``shape`` in {0, 1 / keep}.  Element e (row-major over the
    whole array; ``offset`` = the first element when only a piece is wanted) is kept when
    ``splitmix64(key + G (e + 1)) >> 40 < ceil(keep 2^24)``, key = :func:`mask_key`.  keep = 1 keeps everything."""
    n = int(np.prod(shape, dtype=np.int64))
    bits = keep_bits(mask_key(seed, step, site), int(offset), n, keep_threshold(keep))
    return (bits.astype(np.float64) / float(keep)).reshape(shape)


def adam_lr_t(lr, t):
    return float(lr) * math.sqrt(1.0 - BETA2 ** t) / (1.0 - BETA1 ** t)


def adam_reference(w, g, m, v, t, lr):
    """One Adam update in TensorFlow's form at step t >= 1 (float64) -> (w, m, v)"""
    m = BETA1 * m + (1.0 - BETA1) * g
    v = BETA2 * v + (1.0 - BETA2) * g * g
    return w - adam_lr_t(lr, t) * m / (np.sqrt(v) + EPSILON), m, v


# ------------------------------------------------------------------------------------------------- the step, restated
def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def build_embedding(w, d):
    """The dense Emb [V, E] of a dump-shaped weight dict (float64)"""
    if d["kind"] == "tied":
        return np.asarray(w["LM"], dtype=np.float64)
    if d["kind"] == "vtable":
        parts = [np.asarray(w["LM0"], dtype=np.float64)]
        for i in range(1, len(d["segs"])):
            parts.append(np.asarray(w["LM%d" % i], dtype=np.float64) @ np.asarray(w["VT%d" % i], dtype=np.float64))
        return np.concatenate(parts, axis=0)
    emb = np.zeros((d["V"], d["E"]))
    c0 = 0
    for i, (size, s, e) in enumerate(d["segs"]):
        emb[s:e, c0:c0 + size] = w["LM"][i]
        c0 += size
    return emb


def embedding_grads(w, d, demb):
    """dEmb [V, E] -> the gradients of the embedding tensors (the factorisation's chain rule)"""
    g = {}
    if d["kind"] == "tied":
        g["LM"] = demb
    elif d["kind"] == "vtable":
        for i, (size, s, e) in enumerate(d["segs"]):
            if i == 0:
                g["LM0"] = demb[s:e].copy()
            else:
                g["LM%d" % i] = demb[s:e] @ np.asarray(w["VT%d" % i], dtype=np.float64).T
                g["VT%d" % i] = np.asarray(w["LM%d" % i], dtype=np.float64).T @ demb[s:e]
    else:
        g["LM"], c0 = [], 0
        for size, s, e in d["segs"]:
            g["LM"].append(demb[s:e, c0:c0 + size].copy())
            c0 += size
    return g


class _StepperBase:
    """what the epoch loop needs of a stepper: reset_state, step_async, losses, weights, load_weights"""

    def _setup(self, cfg, batch_size, num_steps, lr, dropout, norm_weight, seed, n_out):
        self.cfg = cfg
        self.d = model_dims(cfg, n_out)
        self.B, self.T = int(batch_size), int(num_steps)
        self.lr, self.keep = float(lr), float(dropout)
        self.norm_weight = float(norm_weight) if cfg.get("self_norm") else 0.0
        self.seed = int(seed)
        self.t = 0                         # Adam steps taken; also the step counter of the dropout masks

    def _check_batch(self, x, y):
        x, y = np.asarray(x), np.asarray(y)
        if x.shape != (self.B, self.T) or y.shape != (self.B, self.T):
            raise ValueError("a step takes inputs and targets [%d, %d] (got %s, %s)" % (self.B, self.T, x.shape, y.shape))
        for a in (x, y):
            if a.min() < 0 or a.max() >= self.d["V"]:
                raise ValueError("word id outside [0, %d)" % self.d["V"])
        # time-major rows: row = t B + b
        return np.ascontiguousarray(x.T).reshape(-1).astype(np.int64), np.ascontiguousarray(y.T).reshape(-1).astype(np.int64)

    def step(self, x, y, train=True):
        """one chunk: -> ce (the mean cross-entropy of its B T tokens); with ``train`` the weights are updated"""
        self.step_async(x, y, train)
        return float(self.losses()[-1])


class ReferenceStepper(_StepperBase):
    """The training step in numpy float64 (module docstring).  ``weights``: a dump-shaped dict (init_weights)."""

    def __init__(self, cfg, weights, batch_size, num_steps, lr=1e-3, dropout=1.0, norm_weight=0.1, seed=0):
        self._setup(cfg, batch_size, num_steps, lr, dropout, norm_weight, seed, np.asarray(weights["b2"]).shape[0])
        self.load_weights(weights)
        self.m = _map(self.w, np.zeros_like)
        self.v = _map(self.w, np.zeros_like)
        self._g = None
        self._losses = []
        self.reset_state()

    def load_weights(self, weights):
        self.w = _map(weights, lambda a: np.array(a, dtype=np.float64))

    def weights(self):
        return _map(self.w, lambda a: a.astype(np.float32))

    def grads(self):
        """the last training step's gradients, dump-shaped (float64)"""
        return self._g

    def reset_state(self):
        self.h = np.zeros((self.B, self.d["H"]))
        self.c = np.zeros((self.B, self.d["H"]))
        self._losses = []

    def set_state(self, h, c):
        self.h, self.c = np.array(h, dtype=np.float64), np.array(c, dtype=np.float64)

    def losses(self):
        out = np.array(self._losses, dtype=np.float64)
        bad = np.nonzero(~np.isfinite(out))[0]
        if len(bad):
            raise NonFiniteLoss(bad[0])
        return out

    def step_async(self, x, y, train=True):
        ids, tgt = self._check_batch(x, y)
        w, d, B, T = self.w, self.d, self.B, self.T
        H, E, N = d["H"], d["E"], self.B * self.T
        keep = self.keep if train else 1.0
        mask_in = dropout_mask(self.seed, self.t, SITE_INPUT, (N, E), keep)
        mask_out = dropout_mask(self.seed, self.t, SITE_OUTPUT, (N, H), keep)
        emb = build_embedding(w, d)
        HM = np.concatenate([w["HM" + g] for g in GATES], axis=1)
        IM = np.concatenate([w["IM" + g] for g in GATES], axis=1)
        b = np.concatenate([w["b" + g] for g in GATES])
        X = mask_in * emb[ids]
        hs = np.zeros((T + 1, B, H))
        cs = np.zeros((T + 1, B, H))
        hs[0], cs[0] = self.h, self.c
        gates = np.zeros((T, B, 4 * H))
        for t in range(T):
            z = hs[t] @ HM + X[t * B:(t + 1) * B] @ IM + b
            gi, gf, go, gg = _sigmoid(z[:, :H]), _sigmoid(z[:, H:2 * H]), _sigmoid(z[:, 2 * H:3 * H]), np.tanh(z[:, 3 * H:])
            gates[t] = np.concatenate([gi, gf, go, gg], axis=1)
            cs[t + 1] = cs[t] * gf + gg * gi
            hs[t + 1] = np.tanh(cs[t + 1]) * go
        R = mask_out * hs[1:].reshape(N, H)
        P = R @ w["PM"]
        Y = P @ emb.T + w["b2"]
        mx = Y.max(axis=1)
        lse = mx + np.log(np.exp(Y - mx[:, None]).sum(axis=1))
        ce = float(np.mean(lse - Y[np.arange(N), tgt]))
        with np.errstate(over="ignore"):
            finite = np.isfinite(ce + self.norm_weight * float(np.mean(lse * lse)))
        self._losses.append(ce if finite else float("inf"))     # ce is what is reported; a non-finite training LOSS stops the run
        self.h, self.c = hs[T].copy(), cs[T].copy()
        if not train:
            return
        # ---- backward
        dY = self._dy(Y, lse, ids, tgt)
        dY /= N
        g = {"b2": dY.sum(axis=0)}
        demb = dY.T @ P
        dP = dY @ emb
        del dY, Y
        g["PM"] = R.T @ dP
        dR = (dP @ w["PM"].T) * mask_out
        dZ = np.zeros((T, B, 4 * H))
        dc = np.zeros((B, H))
        dh_next = np.zeros((B, H))
        for t in range(T - 1, -1, -1):
            gi, gf, go, gg = (gates[t][:, k * H:(k + 1) * H] for k in range(4))
            dh = dR[t * B:(t + 1) * B] + dh_next
            tc = np.tanh(cs[t + 1])
            dcc = dc + dh * go * (1.0 - tc * tc)
            dZ[t] = np.concatenate([dcc * gg * gi * (1.0 - gi), dcc * cs[t] * gf * (1.0 - gf), dh * tc * go * (1.0 - go),
                                    dcc * gi * (1.0 - gg * gg)], axis=1)
            dc = dcc * gf
            dh_next = dZ[t] @ HM.T
        dZ = dZ.reshape(N, 4 * H)
        dHM, dIM, db = hs[:T].reshape(N, H).T @ dZ, X.T @ dZ, dZ.sum(axis=0)
        for k, gname in enumerate(GATES):
            g["HM" + gname], g["IM" + gname], g["b" + gname] = dHM[:, k * H:(k + 1) * H], dIM[:, k * H:(k + 1) * H], db[k * H:(k + 1) * H]
        np.add.at(demb, ids, (dZ @ IM.T) * mask_in)
        g.update(embedding_grads(w, d, demb))
        self._g = g
        self._update(g)

    def _dy(self, Y, lse, ids, tgt):
        """N times the gradient of a training step's loss in its logits Y [N, V] (a subclass trains on another loss:
        jlm_amd/distill.py)"""
        N = Y.shape[0]
        dY = np.exp(Y - lse[:, None])
        if self.norm_weight:
            dY *= (1.0 + 2.0 * self.norm_weight * lse)[:, None]
        dY[np.arange(N), tgt] -= 1.0
        return dY

    def _update(self, g):
        """the tail of a training step: Adam over every tensor (a subclass updates something else: jlm_amd/finetune.py)"""
        w = self.w
        self.t += 1
        for key, idx, a in list(_items(w)):
            if idx is None:
                w[key], self.m[key], self.v[key] = adam_reference(a, g[key], self.m[key], self.v[key], self.t, self.lr)
            else:
                w[key][idx], self.m[key][idx], self.v[key][idx] = adam_reference(a, g[key][idx], self.m[key][idx], self.v[key][idx],
                                                                                 self.t, self.lr)


# ------------------------------------------------------------------------------------------------- the device
def _signed64(z):
    return z - (1 << 64) if z >= 1 << 63 else z


def vocabulary_segments(d):
    """model_dims' dict -> the vocabulary as the device meets it: list of (start, end, width k, block key, how its projected rows
    Q [N, k] come about: direct | cols | factored, first column of P, VT key or None)"""
    V, E, segs = d["V"], d["E"], []
    if d["kind"] == "tied":
        segs.append((0, V, E, ("LM", None), "direct", 0, None))
    c0 = 0
    for i, (size, s, e) in enumerate(d["segs"]):
        if d["kind"] == "dsoftmax":
            segs.append((s, e, size, ("LM", i), "cols", c0, None))
            c0 += size
        elif i == 0:
            segs.append((s, e, size, ("LM0", None), "direct", 0, None))
        else:
            segs.append((s, e, size, ("LM%d" % i, None), "factored", 0, ("VT%d" % i, None)))
    return segs


def window_pieces(segs, v0, v1):
    """the words [v0, v1) cut where a segment ends: [(segment, piece start, piece length)]"""
    return [(si, max(v0, sg[0]), min(v1, sg[1]) - max(v0, sg[0])) for si, sg in enumerate(segs) if sg[0] < v1 and sg[1] > v0]


class DeviceStepper(_StepperBase):
    """The training step on the GPU (csrc/jlm_train.hip through torch.ops.jlm.train_*): the interface of :class:`ReferenceStepper`.
    One step is a fixed launch sequence on the current stream; nothing comes back to the host before :meth:`losses`."""

    def __init__(self, cfg, weights, batch_size, num_steps, lr=1e-3, dropout=1.0, norm_weight=0.1, seed=0, device=None, chunk_bytes=None):
        import torch
        from . import _lib, ops as _ops
        self.torch = torch
        self.dev = device if device is not None else _lib.require_gpu()
        self.ops = _ops.backend()
        self._setup(cfg, batch_size, num_steps, lr, dropout, norm_weight, seed, np.asarray(weights["b2"]).shape[0])
        d, B, T = self.d, self.B, self.T
        V, H, E, N = d["V"], d["H"], d["E"], self.B * self.T
        if N > 65535:
            raise ValueError("batch_size * num_steps must be <= 65535 (got %d)" % N)
        # the flat parameter buffer: the four gate matrices side by side, every tensor at a 16-byte boundary
        layout, off = [], 0
        shapes = [("HM", None, (H, 4 * H)), ("IM", None, (E, 4 * H)), ("b", None, (4 * H,))]
        shapes += [(k, i, s) for k, i, s, _f in weight_shapes(cfg, V) if k[:2] not in ("HM", "IM") and k not in ("bi", "bf", "bo", "bg")]
        for key, idx, shape in shapes:
            n = int(np.prod(shape))
            layout.append((key, idx, shape, off, n))
            off += (n + 3) // 4 * 4
        self.layout, self.n_flat = layout, off
        f32 = torch.float32
        with torch.cuda.device(self.dev):
            z = lambda *s, dtype=f32: torch.zeros(s, device=self.dev, dtype=dtype)
            self.W, self.G, self.M, self.Vv = z(off), z(off), z(off), z(off)
            self.p = {(k, i): self.W[o:o + n].view(*s) for k, i, s, o, n in layout}
            self.g = {(k, i): self.G[o:o + n].view(*s) for k, i, s, o, n in layout}
            # the dense Emb the input rows are gathered from (tied: LM itself; else assembled before every step)
            self.emb = self.p[("LM", None)] if d["kind"] == "tied" else z(V, E)
            # the vocabulary as segments (start, end, width k, block, how its projected rows Q [N, k] come about, first column, VT):
            #   direct    Q = P                      (tied LM; LM0 of a V_table model)
            #   cols      Q = P[:, c0:c0 + k]        (a D_softmax block)
            #   factored  Q = P VT^T                 (V_table segments i > 0: the cost stays V_i k, as in inference)
            self.segs, self.Q, self.dQ, self.D = vocabulary_segments(d), {}, {}, {}
            for i, (s, e, size, _blk, kind, _c0, _vt) in enumerate(self.segs):
                if kind == "factored":
                    self.Q[i], self.dQ[i], self.D[i] = z(N, size), z(N, size), z(e - s, E)
            self.X, self.dX, self.P, self.dP = z(N, E), z(N, E), z(N, E), z(N, E)
            self.Z, self.dZ = z(N, 4 * H), z(N, 4 * H)
            self.Hs, self.Cs = z((T + 1) * B, H), z((T + 1) * B, H)
            self.R, self.dR = z(N, H), z(N, H)
            self.dc, self.dh = z(B, H), z(B, H)
            self.run_m, self.run_s, self.tgt = z(N), z(N), z(N)
            budget = TRAIN_CHUNK_BYTES if chunk_bytes is None else int(chunk_bytes)
            # a multiple of 64 words: every window then starts on a granule of train_lse_update, and the normaliser does not depend on Vc
            self.Vc = int(min(V, max(64, budget // (4 * N) // 64 * 64)))
            self.Y = z(N, self.Vc)
            self.flag = z(1, dtype=torch.int32)
            self.ce = z(256, dtype=torch.float64)
        self.n_ce = 0
        self.timed, self._marks = False, []      # tools/train_bench.py: HIP events at the phase boundaries of a step
        self.load_weights(weights)

    def _mark(self, name):
        if self.timed:
            ev = self.torch.cuda.Event(enable_timing=True)
            ev.record()
            self._marks.append((name, ev))

    def phase_ms(self):
        """with ``timed`` set: milliseconds per phase of the steps since the last call (summed), after one synchronisation"""
        self.torch.cuda.synchronize(self.dev)
        out = {}
        for (_n0, a), (name, b) in zip(self._marks, self._marks[1:]):
            if name != "start":
                out[name] = out.get(name, 0.0) + a.elapsed_time(b)
        self._marks = []
        return out

    # ---- weights in and out
    def _split(self, flat):
        """a host copy of a flat buffer -> the dump-shaped dict (the gate matrices split again)"""
        H, out = self.d["H"], {}
        for key, idx, shape, off, n in self.layout:
            a = flat[off:off + n].reshape(shape)
            if key in ("HM", "IM", "b"):
                for k, gname in enumerate(GATES):
                    out[key + gname] = np.ascontiguousarray(a[..., k * H:(k + 1) * H])
            elif idx is None:
                out[key] = a.copy()
            else:
                out.setdefault(key, []).append(a.copy())
        return out

    def load_weights(self, weights):
        flat = np.zeros(self.n_flat, dtype=np.float32)
        for key, idx, shape, off, n in self.layout:
            if key in ("HM", "IM", "b"):
                a = np.concatenate([np.asarray(weights[key + gname], dtype=np.float32) for gname in GATES], axis=-1)
            else:
                a = np.asarray(weights[key] if idx is None else weights[key][idx], dtype=np.float32)
            if a.shape != tuple(shape):
                raise ValueError("tensor %s has shape %s, the model needs %s" % (key, a.shape, tuple(shape)))
            flat[off:off + n] = a.reshape(-1)
        self.W.copy_(self.torch.from_numpy(flat))

    def weights(self):
        return self._split(self.W.cpu().numpy())

    def grads(self):
        return self._split(self.G.cpu().numpy())

    def reset_state(self):
        self.Hs[:self.B].zero_()
        self.Cs[:self.B].zero_()
        self.n_ce = 0

    def set_state(self, h, c):
        t = self.torch
        self.Hs[:self.B].copy_(t.from_numpy(np.ascontiguousarray(h, dtype=np.float32)))
        self.Cs[:self.B].copy_(t.from_numpy(np.ascontiguousarray(c, dtype=np.float32)))

    def losses(self):
        """the ce of every step since reset_state (one read-back); NonFiniteLoss names the first step that is not finite"""
        out = self.ce[:self.n_ce].cpu().numpy().copy()
        if int(self.flag.item()) or not np.isfinite(out).all():
            bad = np.nonzero(~np.isfinite(out))[0]
            raise NonFiniteLoss(bad[0] if len(bad) else 0)
        return out

    def _update(self):
        """the tail of a training step, inside the step's device context: Adam over the flat parameter buffer (a subclass updates
        something else: jlm_amd/finetune.py)"""
        self.t += 1
        self.ops.train_adam(self.W, self.G, self.M, self.Vv, self.n_flat, adam_lr_t(self.lr, self.t), self.flag)
        self._mark("adam")

    def _gemm(self, *args):
        """every contraction of a step (a subclass routes some of them to another launch form: jlm_amd/dyneval.py)"""
        self.ops.train_gemm(*args)

    # ---- the embedding's forms
    def _assemble_embedding(self):
        d, O, E = self.d, self.ops, self.d["E"]
        if d["kind"] == "vtable":
            for i, (size, s, e) in enumerate(d["segs"]):
                if i == 0:
                    self.emb[s:e].copy_(self.p[("LM0", None)])
                else:
                    self._gemm(self.p[("LM%d" % i, None)], size, 1, self.p[("VT%d" % i, None)], E, 1, self.emb[s:e], E, e - s, E, size, False,
                                 None)
        elif d["kind"] == "dsoftmax":
            c0 = 0
            for i, (size, s, e) in enumerate(d["segs"]):
                self.emb[s:e, c0:c0 + size].copy_(self.p[("LM", i)])
                c0 += size

    def _q(self, si):
        """segment si -> (its projected rows Q, their leading dimension, the gradient buffer of the same shape)"""
        _s, _e, k, _blk, kind, c0, _vt = self.segs[si]
        if kind == "factored":
            return self.Q[si], k, self.dQ[si]
        if kind == "cols":
            return self.P[:, c0:c0 + k], self.d["E"], self.dP[:, c0:c0 + k]
        return self.P, self.d["E"], self.dP

    def _windows(self):
        """the vocabulary in windows of at most Vc words (the logits scratch); a window is cut where a segment ends:
        -> list of (v0, n, [(segment, piece start, piece length)])"""
        out = []
        for v0 in range(0, self.d["V"], self.Vc):
            v1 = min(self.d["V"], v0 + self.Vc)
            out.append((v0, v1 - v0, window_pieces(self.segs, v0, v1)))
        return out

    def _logits(self, v0, pieces):
        """Y[:, a - v0 : a - v0 + n] = Q block[a:a + n]^T + b2[a:a + n] for every piece (a, n) of the window that starts at v0"""
        N = self.B * self.T
        for si, a, n in pieces:
            s, _e, k, blk, _kind, _c0, _vt = self.segs[si]
            Q, ldq, _dq = self._q(si)
            self._gemm(Q, ldq, 1, self.p[blk][a - s:a - s + n], 1, k, self.Y[:, a - v0:], self.Vc, N, n, k, False,
                                self.p[("b2", None)][a:a + n])

    def _vocabulary_loss(self, train, ids_d, tgt_d):
        """From P and the factored Q to the step's ce slot and, with ``train``, db2, dBlock, dVT and dP: the chunked vocabulary loss,
        inside the step's device context (a subclass trains on another loss: jlm_amd/distill.py)"""
        O, N, Vc = self.ops, self.B * self.T, self.Vc
        windows = self._windows()
        s, nw2 = 1.0 / N, 2.0 * self.norm_weight
        for wi, (v0, n, pieces) in enumerate(windows):
            self._logits(v0, pieces)
            O.train_lse_update(self.Y, Vc, n, N, self.run_m, self.run_s, wi == 0)
            if not train:            # the target's logit is read on the way (the dy written here is never used)
                O.train_dy(self.Y, Vc, n, v0, N, self.run_m, self.run_s, tgt_d, self.tgt, s, nw2)
        if train:
            # ---- second pass: dy of a window in place, and the products it feeds, segment by segment
            for v0, n, pieces in windows:
                if len(windows) > 1:
                    self._logits(v0, pieces)
                O.train_dy(self.Y, Vc, n, v0, N, self.run_m, self.run_s, tgt_d, self.tgt, s, nw2)
                self._dy_products(v0, n, pieces)
        O.train_ce(self.run_m, self.run_s, self.tgt, N, self.norm_weight, self.ce[self.n_ce:], self.flag)

    def _dy_products(self, v0, n, pieces):
        """what the dy of a window (in Y) feeds: db2 of its words, then per piece dBlock, dQ and, where a factored segment ends, dVT, dP"""
        O, p, g, N, E, Vc = self.ops, self.p, self.g, self.B * self.T, self.d["E"], self.Vc
        O.train_colsum(self.Y, Vc, N, n, g[("b2", None)][v0:v0 + n], False)
        for si, a, m in pieces:
            s0, e0, k, blk, kind, _c0, vt = self.segs[si]
            Q, ldq, dQ = self._q(si)
            dy = self.Y[:, a - v0:]
            self._gemm(dy, 1, Vc, Q, ldq, 1, g[blk][a - s0:a - s0 + m], k, m, k, N, False, None)      # dBlock = dy^T Q (TN)
            self._gemm(dy, Vc, 1, p[blk][a - s0:a - s0 + m], k, 1, dQ, ldq, N, k, m, a > s0, None)    # dQ (+)= dy Block (NN)
            if kind == "factored" and a + m == e0:
                self._gemm(dQ, 1, k, self.P, E, 1, g[vt], E, k, E, N, False, None)                   # dVT_i = dQ_i^T P (TN)
                self._gemm(dQ, k, 1, p[vt], E, 1, self.dP, E, N, E, k, True, None)                   # dP += dQ_i VT_i (NN)

    def step_async(self, x, y, train=True):
        torch, O, d, B, T = self.torch, self.ops, self.d, self.B, self.T
        ids, tgt = self._check_batch(x, y)
        V, H, E, N = d["V"], d["H"], d["E"], B * T
        keep = self.keep if train else 1.0
        thr, scale = keep_threshold(keep), 1.0 / keep
        key_in, key_out = _signed64(mask_key(self.seed, self.t, SITE_INPUT)), _signed64(mask_key(self.seed, self.t, SITE_OUTPUT))
        p, g = self.p, self.g
        HM, IM = p[("HM", None)], p[("IM", None)]
        with torch.cuda.device(self.dev):
            ids_d = torch.from_numpy(ids.astype(np.int32)).to(self.dev)
            tgt_d = torch.from_numpy(tgt.astype(np.int32)).to(self.dev)
            if self.n_ce >= self.ce.numel():
                self.ce = torch.cat([self.ce, torch.zeros_like(self.ce)])
            # ---- forward
            self._mark("start")
            self._assemble_embedding()
            O.train_embed_rows(self.emb, E, V, ids_d, N, E, self.X, key_in, thr, scale)
            self._gemm(self.X, E, 1, IM, 4 * H, 1, self.Z, 4 * H, N, 4 * H, E, False, p[("b", None)])
            self._mark("inputs")
            for t in range(T):
                rows, nxt = slice(t * B, (t + 1) * B), slice((t + 1) * B, (t + 2) * B)
                self._gemm(self.Hs[rows], H, 1, HM, 4 * H, 1, self.Z[rows], 4 * H, B, 4 * H, H, True, None)
                O.train_cell_fwd(self.Z[rows], self.Cs[rows], self.Cs[nxt], self.Hs[nxt], self.R[rows], B, H, t * B, key_out, thr, scale)
            self._mark("lstm_forward")
            self._gemm(self.R, H, 1, p[("PM", None)], E, 1, self.P, E, N, E, H, False, None)
            for si, sg in enumerate(self.segs):
                if sg[4] == "factored":                                                                            # Q_i = P VT_i^T (NT)
                    self._gemm(self.P, E, 1, p[sg[6]], 1, E, self.Q[si], sg[2], N, sg[2], E, False, None)
            self._vocabulary_loss(train, ids_d, tgt_d)
            self.n_ce += 1
            self._mark("vocabulary")
            if train:
                self._gemm(self.R, 1, H, self.dP, E, 1, g[("PM", None)], E, H, E, N, False, None)                # dPM = R^T dP (TN)
                self._gemm(self.dP, E, 1, p[("PM", None)], 1, E, self.dR, H, N, H, E, False, None)              # dr = dP PM^T (NT)
                self.dc.zero_()
                self._mark("projection_backward")
                for t in range(T - 1, -1, -1):
                    rows, nxt = slice(t * B, (t + 1) * B), slice((t + 1) * B, (t + 2) * B)
                    O.train_cell_bwd(self.Z[rows], self.Cs[nxt], self.Cs[rows], self.dR[rows], self.dh if t < T - 1 else None, self.dc,
                                     self.dZ[rows], B, H, t * B, key_out, thr, scale)
                    if t:
                        self._gemm(self.dZ[rows], 4 * H, 1, HM, 1, 4 * H, self.dh, H, B, H, 4 * H, False, None)  # dh_prev = dz HM^T (NT)
                self._mark("lstm_backward")
                self._gemm(self.Hs, 1, H, self.dZ, 4 * H, 1, g[("HM", None)], 4 * H, H, 4 * H, N, False, None)   # dHM = h_prev^T dz (TN)
                self._gemm(self.X, 1, E, self.dZ, 4 * H, 1, g[("IM", None)], 4 * H, E, 4 * H, N, False, None)    # dIM = x^T dz (TN)
                O.train_colsum(self.dZ, 4 * H, N, 4 * H, g[("b", None)], False)
                self._gemm(self.dZ, 4 * H, 1, IM, 1, 4 * H, self.dX, E, N, E, 4 * H, False, None)               # dx = dz IM^T (NT)
                ids_sorted, perm = torch.sort(ids_d, stable=True)
                for si, (s0, e0, k, blk, kind, c0, vt) in enumerate(self.segs):
                    if kind != "factored":           # dBlock[w] += the rows that read word w (their columns of this block)
                        O.train_scatter_rows(self.dX, E, c0, k, E, ids_sorted, perm, N, g[blk], k, s0, e0, key_in, thr, scale)
                    else:                            # through the factorisation: dLM_i += D VT_i^T, dVT_i += LM_i^T D
                        D = self.D[si]
                        D.zero_()
                        O.train_scatter_rows(self.dX, E, 0, E, E, ids_sorted, perm, N, D, E, s0, e0, key_in, thr, scale)
                        self._gemm(D, E, 1, p[vt], 1, E, g[blk], k, e0 - s0, k, E, True, None)
                        self._gemm(p[blk], 1, k, D, E, 1, g[vt], E, k, E, e0 - s0, True, None)
                self._mark("weight_gradients")
                self._update()
            self.Hs[:B].copy_(self.Hs[T * B:])
            self.Cs[:B].copy_(self.Cs[T * B:])


# ------------------------------------------------------------------------------------------------- the driver
def run_epoch(stepper, data, batch_size, num_steps, train, verbose=10):
    """train/model.py run_epoch: one pass over ``data`` (an id stream) from the zero state -> exp(mean over steps of ce).  The losses
    are read back at the end and every ``verbose`` steps of a training pass (0: at the end only), which is where a non-finite loss
    stops the run."""
    from .score import stream_layout
    x, y = stream_layout(data, batch_size, num_steps)
    stepper.reset_state()
    n_chunks = x.shape[1] // num_steps
    for i in range(n_chunks):
        cols = slice(i * num_steps, (i + 1) * num_steps)
        stepper.step_async(x[:, cols], y[:, cols], train)
        if train and verbose and i % verbose == 0:
            stepper.losses()
    return float(np.exp(np.mean(stepper.losses())))


def fit(stepper, train_data, dev_data, test_data, parameters, log=print, save=None, verbose=10, best_pp=float("inf")):
    """train/train.py:80-102: per epoch a training and a validation pass; ``save(weights)`` when the validation perplexity improves;
    stop when epoch - best_epoch > early_stopping; then the test pass with the current weights, and one with the saved best.
    ``best_pp``: the validation perplexity an epoch has to beat to be saved (fine-tuning starts from a model that has one).
    -> dict(best_epoch, best_valid_pp, history = [(train_pp, valid_pp)], test_pp, best_test_pp, best_weights)"""
    B, T = int(parameters["batch_size"]), int(parameters["num_steps"])
    best_pp, best_epoch, best_weights, history = float(best_pp), 0, None, []
    epoch = 0
    for epoch in range(int(parameters["max_epochs"])):
        log("Epoch {}".format(epoch))
        start = time.time()
        try:
            train_pp = run_epoch(stepper, train_data, B, T, True, verbose)
        except NonFiniteLoss as e:
            raise NonFiniteLoss(e.step, epoch)
        log("Training perplexity: {}".format(train_pp))
        log("Total Training time: {}".format(time.time() - start))
        valid_pp = run_epoch(stepper, dev_data, B, T, False)
        log("Validation perplexity: {}".format(valid_pp))
        history.append((train_pp, valid_pp))
        if valid_pp < best_pp:
            best_pp, best_epoch, best_weights = valid_pp, epoch, stepper.weights()
            if save is not None:
                save(best_weights)
        if epoch - best_epoch > int(parameters["early_stopping"]):
            break
        log("Total time: {}".format(time.time() - start))
    test_pp = run_epoch(stepper, test_data, B, T, False)
    log("Test perplexity: {}".format(test_pp))
    best_test_pp = test_pp
    if best_weights is not None and best_epoch != epoch:
        stepper.load_weights(best_weights)
        best_test_pp = run_epoch(stepper, test_data, B, T, False)
    log("Test perplexity of the saved weights (epoch {}): {}".format(best_epoch, best_test_pp))
    return dict(best_epoch=best_epoch, best_valid_pp=best_pp, history=history, test_pp=test_pp, best_test_pp=best_test_pp,
                best_weights=best_weights, last_epoch=epoch)


def next_experiment_id():
    """the next unused integer directory under config.experiment_path (sacred's FileStorageObserver numbering)"""
    used = [int(n) for n in os.listdir(_config.experiment_path) if n.isdigit()] if os.path.isdir(_config.experiment_path) else []
    return max(used) + 1 if used else 1


def load_corpus(vocab, debug=False):
    """Corpus.encode_corpus (train/data.py:54-70) over data/train.txt, dev.txt, test.txt -> three id streams"""
    from .perplexity import encode_lines, read_lines
    out = []
    for name in ("train.txt", "dev.txt", "test.txt"):
        sents, _unk = encode_lines(read_lines(os.path.join(_config.data_path, name), 1024 * 100 if debug else 0), vocab)
        out.append(np.array([i for s in sents for i in s], dtype=np.int32))
    return out


def write_experiment(experiment_id, parameters, weights):
    d = os.path.join(_config.experiment_path, str(experiment_id))
    os.makedirs(os.path.join(d, "weights"), exist_ok=True)
    with open(os.path.join(d, "config.json"), "wt") as f:
        f.write(json.dumps(parameters))
    if weights is not None:
        with open(os.path.join(d, "weights", "lstm_weights.pkl"), "wb") as f:
            pickle.dump(weights, f)


last_result = {}                      # the last train_experiment call's fit() result (without the weights)


def train_experiment(parameters, root=None, log=print, stepper=None, initial_weights=None, verbose=10):
    """Train one experiment (train/train.py ``train_RNNLM``) and write it: -> experiment id.
    ``parameters``: the dict of train/train.py:13-36 (missing keys take its defaults; ``gpu_id`` is the device index -- the current
    device where the machine has no such index -- and ``debug`` reads the first 1024 * 100 lines).  ``stepper``: None = :class:`DeviceStepper`, ``"reference"`` = :class:`ReferenceStepper` (the tests'
    CPU run of a tiny model), or a callable ``(cfg, weights, batch_size, num_steps, lr, dropout, norm_weight, seed) -> stepper``.
    ``initial_weights``: a dump-shaped dict instead of :func:`init_weights` (tests)."""
    from .data import CharVocab, Vocab
    p = check_parameters(parameters)
    if root:
        _config.set_root(root)
    vocab = (CharVocab if p["char_rnn"] else Vocab)(p["vocab_size"])
    n_out = len(vocab)
    if not p["char_rnn"] and n_out != p["vocab_size"]:
        raise ValueError("the lexicon gives %d words, vocab_size asks for %d" % (n_out, p["vocab_size"]))
    train_data, dev_data, test_data = load_corpus(vocab, p["debug"])
    weights = initial_weights if initial_weights is not None else init_weights(p, n_out, p["tf_random_seed"])
    kw = dict(batch_size=p["batch_size"], num_steps=p["num_steps"], lr=p["lr"], dropout=p["dropout"], norm_weight=p["norm_weight"],
              seed=p["tf_random_seed"])
    if stepper is None:
        import torch
        from . import _lib
        _lib.require_gpu()
        dev = torch.device("cuda", int(p["gpu_id"]) if int(p["gpu_id"]) < torch.cuda.device_count() else torch.cuda.current_device())
        st = DeviceStepper(p, weights, device=dev, **kw)
    elif stepper == "reference":
        st = ReferenceStepper(p, weights, **kw)
    else:
        st = stepper(p, weights, **kw)
    exp_id = next_experiment_id()
    write_experiment(exp_id, p, None)
    result = fit(st, train_data, dev_data, test_data, p, log, lambda w: write_experiment(exp_id, p, w), verbose)
    last_result.clear()
    last_result.update({k: v for k, v in result.items() if k != "best_weights"})
    return exp_id


# ------------------------------------------------------------------------------------------------- command line
def _flag_type(default):
    if isinstance(default, bool):
        return lambda s: {"true": True, "1": True, "yes": True, "false": False, "0": False, "no": False}[s.lower()]
    if isinstance(default, list):
        return json.loads
    return type(default)


def build_parser():
    ap = argparse.ArgumentParser(description="Train the LSTM language model on the device (reference train/train.py)")
    ap.add_argument("--root", default=None, help="artifact root (default: jlm_amd.config's)")
    for key, default in DEFAULTS.items():
        ap.add_argument("--" + key, type=_flag_type(default), default=default,
                        help="train/train.py parameters[%r] (default %s)" % (key, json.dumps(default)))
    return ap


def main(argv=None):
    args = vars(build_parser().parse_args(argv))
    root = args.pop("root")
    return train_experiment(args, root=root)


if __name__ == "__main__":
    main()
