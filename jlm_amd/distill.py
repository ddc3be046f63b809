"""Distillation on the device: train a small student on the soft targets of a large trained teacher
(``distill_experiment``, ``python -m jlm_amd.distill``).

The student's step is jlm_amd/train.py's up to its logits ``y_s`` [N, V].  The teacher is a frozen trained experiment over the same
vocabulary: it reads the same input ids without dropout, from its own carried ``h, c`` (zero where the student's are zero, carried
from chunk to chunk, reset by ``reset_state``), and gives ``y_t`` [N, V].  With temperature tau > 0 and weight alpha in [0, 1]:

  L_s = lse(y_s)          A_s = lse(y_s / tau)          A_t = lse(y_t / tau)
  p   = exp(y_s - L_s)    p^tau = exp(y_s / tau - A_s)  q   = exp(y_t / tau - A_t)
  ce   = mean_rows(L_s - y_s[target])
  kl   = mean_rows sum_w q_w ((y_t[w] / tau - A_t) - (y_s[w] / tau - A_s))       in log space; q_w = 0 adds 0
  loss = (1 - alpha) ce + alpha tau^2 kl + norm_weight mean_rows(L_s^2)          the last term with self_norm
  dy_s = (1 / N) [(1 - alpha) (p - onehot) + 2 norm_weight L_s p + alpha tau (p^tau - q)]

Behind ``dy_s`` the backward pass is train.py's.  No gradient reaches the teacher.  ``losses()`` stays the hard cross-entropy ``ce``, so
``train.fit``, its perplexities and its early stopping work as they are; ``kls()`` gives the ``kl`` of the training steps.  An
evaluation step does not run the teacher.  With alpha = 0 the teacher is never evaluated and a step is train.py's step, launch for
launch.  What is written is an ordinary experiment (plus ``distill.json``): everything that reads one reads a distilled one.
"""
import json
import math
import os

import numpy as np

from . import config as _config
from . import train as _train
from . import weights as _weights
from .train import GATES, NonFiniteLoss, _sigmoid, build_embedding, model_dims


def check_mix(alpha, temperature):
    """-> (alpha, temperature) as floats; ValueError for an alpha outside [0, 1] or a temperature that is not finite and > 0"""
    def number(v):
        return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_))
    if not number(alpha) or not 0.0 <= float(alpha) <= 1.0:                    # a NaN fails both comparisons
        raise ValueError("alpha must be a number in [0, 1] (got %r)" % (alpha,))
    if not number(temperature) or not math.isfinite(float(temperature)) or float(temperature) <= 0.0:
        raise ValueError("temperature must be finite and > 0 (got %r)" % (temperature,))
    return float(alpha), float(temperature)


def teacher_forward(w, d, ids, h, c, B, T):
    """The forward pass of train.ReferenceStepper without dropout (float64): ids [N] time-major, h, c [B, H] -> (Y [N, V], h, c)"""
    H = d["H"]
    emb = build_embedding(w, d)
    HM = np.concatenate([np.asarray(w["HM" + g], dtype=np.float64) for g in GATES], axis=1)
    IM = np.concatenate([np.asarray(w["IM" + g], dtype=np.float64) for g in GATES], axis=1)
    b = np.concatenate([np.asarray(w["b" + g], dtype=np.float64) for g in GATES])
    X = emb[ids]
    hs = np.zeros((T, B, H))
    for t in range(T):
        z = h @ HM + X[t * B:(t + 1) * B] @ IM + b
        gi, gf, go, gg = _sigmoid(z[:, :H]), _sigmoid(z[:, H:2 * H]), _sigmoid(z[:, 2 * H:3 * H]), np.tanh(z[:, 3 * H:])
        c = c * gf + gg * gi
        h = np.tanh(c) * go
        hs[t] = h
    P = hs.reshape(B * T, H) @ np.asarray(w["PM"], dtype=np.float64)
    return P @ emb.T + np.asarray(w["b2"], dtype=np.float64), h, c


def _lse(Y):
    mx = Y.max(axis=1)
    return mx + np.log(np.exp(Y - mx[:, None]).sum(axis=1))


class DistillReferenceStepper(_train.ReferenceStepper):
    """The distilling step in numpy float64 (module docstring): what :class:`DistillDeviceStepper` is judged against."""

    def __init__(self, cfg, weights, teacher_cfg, teacher_weights, batch_size, num_steps, lr=1e-3, dropout=1.0, norm_weight=0.1, seed=0,
                 alpha=0.5, temperature=1.0):
        self.alpha, self.tau = check_mix(alpha, temperature)
        self.td = model_dims(teacher_cfg, np.asarray(teacher_weights["b2"]).shape[0])
        self.tw = _train._map(teacher_weights, lambda a: np.array(a, dtype=np.float64))
        self._kls = []
        _train.ReferenceStepper.__init__(self, cfg, weights, batch_size, num_steps, lr, dropout, norm_weight, seed)
        if self.td["V"] != self.d["V"]:
            raise ValueError("the teacher has %d output words, the student %d" % (self.td["V"], self.d["V"]))

    def reset_state(self):
        _train.ReferenceStepper.reset_state(self)
        self.th = np.zeros((self.B, self.td["H"]))
        self.tc = np.zeros((self.B, self.td["H"]))
        self._kls = []

    def set_teacher_state(self, h, c):
        self.th, self.tc = np.array(h, dtype=np.float64), np.array(c, dtype=np.float64)

    def kls(self):
        """the kl of every training step since reset_state"""
        out = np.array(self._kls, dtype=np.float64)
        bad = np.nonzero(~np.isfinite(out))[0]
        if len(bad):
            raise NonFiniteLoss(bad[0])
        return out

    def _dy(self, Y, lse, ids, tgt):
        if self.alpha == 0.0:
            return _train.ReferenceStepper._dy(self, Y, lse, ids, tgt)
        N, a, tau = Y.shape[0], self.alpha, self.tau
        Yt, self.th, self.tc = teacher_forward(self.tw, self.td, ids, self.th, self.tc, self.B, self.T)
        ls = Y / tau
        ls -= _lse(ls)[:, None]
        lt = Yt / tau
        lt -= _lse(lt)[:, None]
        q = np.exp(lt)
        terms = np.zeros_like(q)
        np.multiply(q, lt - ls, out=terms, where=q != 0)           # q = 0 adds 0; a q that is not a number stays one
        self._kls.append(float(np.mean(terms.sum(axis=1))))
        if not np.isfinite(self._kls[-1]):                 # as on the device: a kl that is not finite stops the run at this step
            self._losses[-1] = float("inf")
        p = np.exp(Y - lse[:, None])
        dY = (1.0 - a) * p
        dY[np.arange(N), tgt] -= 1.0 - a
        if self.norm_weight:
            dY += (2.0 * self.norm_weight * lse)[:, None] * p
        dY += (a * tau) * (np.exp(ls) - q)
        return dY


class DistillDeviceStepper(_train.DeviceStepper):
    """The distilling step on the GPU: train.DeviceStepper with the vocabulary loss of csrc/jlm_train.hip's distill kernels.
    The teacher's parameters sit in device buffers of their own, outside the Adam flat buffer, and its dense Emb is assembled once.
    The student's and the teacher's logits scratches share ``chunk_bytes``: a window holds half as many words as train.py's."""

    def __init__(self, cfg, weights, teacher_cfg, teacher_weights, batch_size, num_steps, lr=1e-3, dropout=1.0, norm_weight=0.1, seed=0,
                 alpha=0.5, temperature=1.0, device=None, chunk_bytes=None):
        self.alpha, self.tau = check_mix(alpha, temperature)
        td = self.td = model_dims(teacher_cfg, np.asarray(teacher_weights["b2"]).shape[0])
        n_out = np.asarray(weights["b2"]).shape[0]
        if td["V"] != n_out:
            raise ValueError("the teacher has %d output words, the student %d" % (td["V"], n_out))
        budget = _train.TRAIN_CHUNK_BYTES if chunk_bytes is None else int(chunk_bytes)
        # alpha = 0 is train.py's step with train.py's windows; otherwise each of the two scratches takes half the budget
        _train.DeviceStepper.__init__(self, cfg, weights, batch_size, num_steps, lr, dropout, norm_weight, seed, device,
                                      budget if self.alpha == 0.0 else budget // 2)
        self.n_kl, self._kl_step = 0, []
        if self.alpha == 0.0:
            return
        torch, B, T, N = self.torch, self.B, self.T, self.B * self.T
        V, H, E = td["V"], td["H"], td["E"]
        with torch.cuda.device(self.dev):
            z = lambda *s, dtype=torch.float32: torch.zeros(s, device=self.dev, dtype=dtype)
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(self.dev)
            # the teacher's tensors as the student's lie in the flat buffer (the four gate matrices side by side), each in its own buffer
            shapes = [("HM", None, (H, 4 * H)), ("IM", None, (E, 4 * H)), ("b", None, (4 * H,))]
            shapes += [(k, i, s) for k, i, s, _f in _train.weight_shapes(teacher_cfg, V)
                       if k[:2] not in ("HM", "IM") and k not in ("bi", "bf", "bo", "bg")]
            tp = {}
            for key, idx, shape in shapes:
                if key in ("HM", "IM", "b"):
                    a = np.concatenate([np.asarray(teacher_weights[key + g], dtype=np.float32) for g in GATES], axis=-1)
                else:
                    a = np.asarray(teacher_weights[key] if idx is None else teacher_weights[key][idx], dtype=np.float32)
                if a.shape != tuple(shape):
                    raise ValueError("teacher tensor %s has shape %s, its configuration needs %s" % (key, a.shape, tuple(shape)))
                tp[(key, idx)] = up(a)
            self.tp, self.tsegs = tp, _train.vocabulary_segments(td)
            self.tQ = {i: z(N, sg[2]) for i, sg in enumerate(self.tsegs) if sg[4] == "factored"}
            self.tX, self.tP, self.tZ, self.tR = z(N, E), z(N, E), z(N, 4 * H), z(N, H)
            self.tHs, self.tCs = z((T + 1) * B, H), z((T + 1) * B, H)
            self.Yt = z(N, self.Vc)
            self.run = z(6, N)
            self.run_m, self.run_s = self.run[0], self.run[1]          # train_ce reads the L_s pair where it always does
            self.kl_row = z(N)
            self.kl = z(256, dtype=torch.float64)
            # the teacher is frozen: its dense Emb is assembled here, once
            if td["kind"] == "tied":
                self.temb = tp[("LM", None)]
            else:
                self.temb = z(V, E)
                c0 = 0
                for i, (size, s, e) in enumerate(td["segs"]):
                    if td["kind"] == "dsoftmax":
                        self.temb[s:e, c0:c0 + size].copy_(tp[("LM", i)])
                        c0 += size
                    elif i == 0:
                        self.temb[s:e].copy_(tp[("LM0", None)])
                    else:
                        self.ops.train_gemm(tp[("LM%d" % i, None)], size, 1, tp[("VT%d" % i, None)], E, 1, self.temb[s:e], E, e - s, E, size,
                                            False, None)

    def teacher_buffers(self):
        """every device buffer that holds a teacher parameter or its dense Emb (tests: their bytes never change)"""
        out = dict(self.tp)
        out[("Emb", None)] = self.temb
        return out

    def reset_state(self):
        _train.DeviceStepper.reset_state(self)
        self.n_kl, self._kl_step = 0, []               # _kl_step[i]: which step of the pass (its ce slot) wrote kl slot i
        if self.alpha != 0.0:
            self.tHs[:self.B].zero_()
            self.tCs[:self.B].zero_()

    def set_teacher_state(self, h, c):
        t = self.torch
        self.tHs[:self.B].copy_(t.from_numpy(np.ascontiguousarray(h, dtype=np.float32)))
        self.tCs[:self.B].copy_(t.from_numpy(np.ascontiguousarray(c, dtype=np.float32)))

    def losses(self):
        """train.DeviceStepper.losses; a kl that is not finite raises the flag word too, and NonFiniteLoss then names the first step
        whose ce or kl is not finite"""
        if self.alpha != 0.0 and int(self.flag.item()):
            ce = self.ce[:self.n_ce].cpu().numpy()
            bad = set(np.nonzero(~np.isfinite(ce))[0].tolist())
            bad.update(self._kl_step[i] for i in np.nonzero(~np.isfinite(self.kl[:self.n_kl].cpu().numpy()))[0])
            raise NonFiniteLoss(min(bad) if bad else 0)
        return _train.DeviceStepper.losses(self)

    def kls(self):
        """the kl of every training step since reset_state (one read-back)"""
        if self.alpha == 0.0:
            return np.zeros(0, dtype=np.float64)
        out = self.kl[:self.n_kl].cpu().numpy().copy()
        bad = np.nonzero(~np.isfinite(out))[0]
        if len(bad):
            raise NonFiniteLoss(self._kl_step[bad[0]])
        return out

    # ---- the teacher's forward pass: the training kernels with everything kept
    def _teacher_forward(self, ids_d):
        O, tp, td, B, T = self.ops, self.tp, self.td, self.B, self.T
        V, H, E, N = td["V"], td["H"], td["E"], B * T
        all_kept = 1 << 24
        O.train_embed_rows(self.temb, E, V, ids_d, N, E, self.tX, 0, all_kept, 1.0)
        O.train_gemm(self.tX, E, 1, tp[("IM", None)], 4 * H, 1, self.tZ, 4 * H, N, 4 * H, E, False, tp[("b", None)])
        for t in range(T):
            rows, nxt = slice(t * B, (t + 1) * B), slice((t + 1) * B, (t + 2) * B)
            O.train_gemm(self.tHs[rows], H, 1, tp[("HM", None)], 4 * H, 1, self.tZ[rows], 4 * H, B, 4 * H, H, True, None)
            O.train_cell_fwd(self.tZ[rows], self.tCs[rows], self.tCs[nxt], self.tHs[nxt], self.tR[rows], B, H, t * B, 0, all_kept, 1.0)
        O.train_gemm(self.tR, H, 1, tp[("PM", None)], E, 1, self.tP, E, N, E, H, False, None)
        for si, sg in enumerate(self.tsegs):
            if sg[4] == "factored":
                O.train_gemm(self.tP, E, 1, tp[sg[6]], 1, E, self.tQ[si], sg[2], N, sg[2], E, False, None)
        self.tHs[:B].copy_(self.tHs[T * B:])
        self.tCs[:B].copy_(self.tCs[T * B:])
        self._mark("teacher_forward")

    def _teacher_logits(self, v0, n):
        """Yt[:, :n] = the teacher's logits of words [v0, v0 + n), cut where ITS segments end"""
        N, E = self.B * self.T, self.td["E"]
        for si, a, m in _train.window_pieces(self.tsegs, v0, v0 + n):
            s, _e, k, blk, kind, c0, _vt = self.tsegs[si]
            if kind == "factored":
                Q, ldq = self.tQ[si], k
            elif kind == "cols":
                Q, ldq = self.tP[:, c0:c0 + k], E
            else:
                Q, ldq = self.tP, E
            self.ops.train_gemm(Q, ldq, 1, self.tp[blk][a - s:a - s + m], 1, k, self.Yt[:, a - v0:], self.Vc, N, m, k, False,
                                self.tp[("b2", None)][a:a + m])

    def _vocabulary_loss(self, train, ids_d, tgt_d):
        if not train or self.alpha == 0.0:
            return _train.DeviceStepper._vocabulary_loss(self, train, ids_d, tgt_d)
        O, torch, N, Vc = self.ops, self.torch, self.B * self.T, self.Vc
        a, tau = self.alpha, self.tau
        if self.n_kl >= self.kl.numel():
            self.kl = torch.cat([self.kl, torch.zeros_like(self.kl)])
        self._teacher_forward(ids_d)
        windows = self._windows()
        for wi, (v0, n, pieces) in enumerate(windows):
            self._logits(v0, pieces)
            self._teacher_logits(v0, n)
            O.train_distill_lse_update(self.Y, Vc, self.Yt, Vc, n, N, 1.0 / tau, self.run, wi == 0)
        for wi, (v0, n, pieces) in enumerate(windows):
            if len(windows) > 1:
                self._logits(v0, pieces)
                self._teacher_logits(v0, n)
            O.train_distill_dy(self.Y, Vc, self.Yt, Vc, n, v0, N, self.run, tgt_d, self.tgt, self.kl_row, 1.0 / N, 2.0 * self.norm_weight,
                               1.0 - a, a * tau, 1.0 / tau, wi == 0)
            self._dy_products(v0, n, pieces)
        O.train_ce(self.run_m, self.run_s, self.tgt, N, self.norm_weight, self.ce[self.n_ce:], self.flag)
        O.train_distill_kl(self.kl_row, N, self.kl[self.n_kl:], self.flag)
        self._kl_step.append(self.n_ce)
        self.n_kl += 1


# ------------------------------------------------------------------------------------------------- the driver
def _softmax_kind(cfg):
    return "V_table" if cfg.get("V_table") else "D_softmax" if cfg.get("D_softmax") else "tied"


last_result = {}                      # the last distill_experiment call's fit() result (without the weights)


def distill_experiment(teacher_id, parameters=None, alpha=0.5, temperature=1.0, root=None, log=print, stepper=None, initial_weights=None,
                       verbose=10):
    """Train a student on the soft targets of experiment ``teacher_id`` and write it as a new experiment: -> its id.
    ``parameters``: train.check_parameters' parameters of the STUDENT (its refusals pass through unchanged).  ``stepper``: None =
    :class:`DistillDeviceStepper`, ``"reference"`` = :class:`DistillReferenceStepper`, or a callable ``(cfg, weights, teacher_cfg,
    teacher_weights, batch_size, num_steps, lr, dropout, norm_weight, seed, alpha, temperature) -> stepper``.
    The new folder holds what ``train_experiment`` writes for the same parameters (``config.json`` byte for byte) and a
    ``distill.json``: teacher id, alpha, temperature, and the teacher's hidden_size, embed_size and softmax kind.  The teacher's
    folder is only read.
    ValueError before any launch and before any file is made: alpha outside [0, 1] or not a number; a temperature that is not finite
    and > 0; a teacher experiment that does not exist; a teacher whose output size is not the student's; a character teacher for a
    word student or the reverse; a teacher with share_embedding=False."""
    from .data import CharVocab, Vocab
    p = _train.check_parameters(dict(parameters or {}))
    alpha, temperature = check_mix(alpha, temperature)
    if root:
        _config.set_root(root)
    tdir = os.path.join(_config.experiment_path, str(teacher_id))
    if not os.path.isfile(os.path.join(tdir, "config.json")):
        raise ValueError("the teacher experiment %s does not exist (no %s)" % (teacher_id, os.path.join(tdir, "config.json")))
    tcfg = _config.load_config_dict(teacher_id)
    if not tcfg.get("share_embedding", True):
        raise ValueError("the teacher has share_embedding=False (an untied projection UM), which is not built")
    if bool(tcfg.get("char_rnn")) != bool(p["char_rnn"]):
        raise ValueError("the teacher is a %s model, the student a %s model" % ("character" if tcfg.get("char_rnn") else "word",
                                                                                 "character" if p["char_rnn"] else "word"))
    try:
        tw = _weights.load_weights(teacher_id, 0, tcfg)
    except FileNotFoundError as e:
        raise ValueError("the teacher experiment %s has no weights (%s)" % (teacher_id, e))
    vocab = (CharVocab if p["char_rnn"] else Vocab)(p["vocab_size"])
    n_out = len(vocab)
    if not p["char_rnn"] and n_out != p["vocab_size"]:
        raise ValueError("the lexicon gives %d words, vocab_size asks for %d" % (n_out, p["vocab_size"]))
    t_out = int(np.asarray(tw["b2"]).shape[0])
    if t_out != n_out:
        raise ValueError("the teacher has %d output words, the student %d" % (t_out, n_out))
    tcfg = dict(tcfg, embedding_seg=[list(s) for s in tcfg.get("embedding_seg", [])])
    model_dims(tcfg, t_out)                                       # its segment list must cut [0, V)
    train_data, dev_data, test_data = _train.load_corpus(vocab, p["debug"])
    weights = initial_weights if initial_weights is not None else _train.init_weights(p, n_out, p["tf_random_seed"])
    kw = dict(batch_size=p["batch_size"], num_steps=p["num_steps"], lr=p["lr"], dropout=p["dropout"], norm_weight=p["norm_weight"],
              seed=p["tf_random_seed"], alpha=alpha, temperature=temperature)
    if stepper is None:
        import torch
        from . import _lib
        _lib.require_gpu()
        dev = torch.device("cuda", int(p["gpu_id"]) if int(p["gpu_id"]) < torch.cuda.device_count() else torch.cuda.current_device())
        st = DistillDeviceStepper(p, weights, tcfg, tw, device=dev, **kw)
    elif stepper == "reference":
        st = DistillReferenceStepper(p, weights, tcfg, tw, **kw)
    else:
        st = stepper(p, weights, tcfg, tw, **kw)
    exp_id = _train.next_experiment_id()
    _train.write_experiment(exp_id, p, None)
    with open(os.path.join(_config.experiment_path, str(exp_id), "distill.json"), "wt") as f:
        f.write(json.dumps(dict(teacher_id=teacher_id, alpha=alpha, temperature=temperature, teacher_hidden_size=int(tcfg["hidden_size"]),
                                teacher_embed_size=int(model_dims(tcfg, t_out)["E"]), teacher_softmax=_softmax_kind(tcfg))))
    result = _train.fit(st, train_data, dev_data, test_data, p, log, lambda w: _train.write_experiment(exp_id, p, w), verbose)
    last_result.clear()
    last_result.update({k: v for k, v in result.items() if k != "best_weights"})
    return exp_id


# ------------------------------------------------------------------------------------------------- command line
def build_parser():
    ap = _train.build_parser()
    ap.description = "Distil a trained experiment into a smaller student on the device"
    ap.add_argument("--teacher", required=True, help="the trained experiment whose soft targets the student learns from")
    ap.add_argument("--alpha", type=float, default=0.5, help="weight of the soft term in [0, 1] (default 0.5; 0 trains on the corpus alone)")
    ap.add_argument("--temperature", type=float, default=1.0, help="softmax temperature of the soft targets (default 1.0)")
    return ap


def main(argv=None):
    args = vars(build_parser().parse_args(argv))
    root, teacher, alpha, temperature = args.pop("root"), args.pop("teacher"), args.pop("alpha"), args.pop("temperature")
    return distill_experiment(teacher, args, alpha=alpha, temperature=temperature, root=root)


if __name__ == "__main__":
    main()
