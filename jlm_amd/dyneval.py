"""Dynamic evaluation on the device: the weights adapt to the text read (``dynamic_perplexity``, ``python -m jlm_amd.perplexity --dynamic``).

Krause, Kahembwe, Murray, Renals, "Dynamic Evaluation of Neural Sequence Models" (2018).  The stream is read in the chunks of
``score.stream_layout`` (what ``train.run_epoch`` reads).  A chunk is scored with the weights as they stand -- its ``ce`` is what a
training step reports, computed before the update -- and then the model takes one gradient step on that chunk, while a decay term pulls
the weights back towards the loaded ones.  The continuous cache (jlm_amd/cache.py) changes no weight; this changes nothing else.

The rule.  theta0: the loaded weights; g: the gradient of the chunk's plain ``ce`` (no self-normalisation term,
no dropout); the hidden state is carried from chunk to chunk and only ``reset_state`` zeroes it.
  rule "sgd"   theta <- theta - lr g + lam (theta0 - theta)
  rule "rms"   theta <- theta - lr g / (RMS + eps) + min(lam RMS / mean(RMS), 1) (theta0 - theta)
               RMS = sqrt(mean over the statistics chunks of g^2) per element, taken at theta0 with the state carried
               (:func:`gradient_stats`); mean(RMS) runs over every parameter (the padding of the device's flat buffer is not counted)

:class:`DynEvalReferenceStepper` is the definition, in numpy float64 on ``train.ReferenceStepper``; :class:`DynEvalDeviceStepper` sits
on ``train.DeviceStepper`` and replaces its Adam launch by ``dyneval_update`` (csrc/jlm_train.hip).  At one stream and chunks of 5 to
20 tokens the step's row-contracting products have a handful of output tiles under a contraction as long as the vocabulary, so the
device stepper also routes those through ``train_gemm_splitk``: the contraction cut into pieces of ``split_kc``, the pieces' tiles
added in order by a second launch.  The result is a pure function of the operands and ``split_kc``.

Settings that diverged or hurt on the project's toy model (V = 600, H = 64; section 23): sgd at lr >= 0.05 on in-domain text, and rms
at eps = 1e-5 with lr = 1e-3.  Tune lr and lam on held-out text (:func:`tune`) before trusting a number.

There is no CPU fallback: ``dynamic_perplexity`` needs the GPU unless it is handed the float64 stepper (``stepper="reference"``).
"""
import math

import numpy as np

from . import config as _config
from . import train as _train
from . import weights as _weights

RULES = ("sgd", "rms")
SPLIT_KC = 128                # the contraction piece of a split product (measured: profiles/dyneval_a_bench.json) ...
SPLIT_MAX_TILES = 32          # ... taken when the product has at most this many 64 x 64 output tiles and K >= 2 SPLIT_KC


class DynEvalSpec:
    """What a dynamic evaluation is asked for (module docstring); :func:`check_spec` judges it."""

    def __init__(self, lr, lam=0.0, rule="sgd", eps=1e-3, batch_size=1, num_steps=5):
        self.lr, self.lam, self.rule, self.eps, self.batch_size, self.num_steps = lr, lam, rule, eps, batch_size, num_steps

    def replace(self, **kw):
        d = dict(lr=self.lr, lam=self.lam, rule=self.rule, eps=self.eps, batch_size=self.batch_size, num_steps=self.num_steps)
        d.update(kw)
        return DynEvalSpec(**d)

    def __repr__(self):
        return "DynEvalSpec(lr=%r, lam=%r, rule=%r, eps=%r, batch_size=%r, num_steps=%r)" % (
            self.lr, self.lam, self.rule, self.eps, self.batch_size, self.num_steps)


def _number(v):
    return not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating))


def _whole(v):
    return not isinstance(v, bool) and isinstance(v, (int, np.integer))


def check_spec(spec, cfg=None, stats=None, n_out=None):
    """ValueError, before anything is launched, for: lr not finite or < 0, lam outside [0, 1), eps <= 0, an unknown rule, a batch size
    or chunk length < 1, rule "rms" without statistics, and -- with the model's ``cfg`` -- statistics whose tensors are not the model's,
    hold something that is not finite and >= 0, or are zero everywhere.  -> the spec"""
    if not isinstance(spec, DynEvalSpec):
        raise ValueError("spec must be a DynEvalSpec (got %r)" % (spec,))
    if not _number(spec.lr) or not math.isfinite(spec.lr) or spec.lr < 0:
        raise ValueError("lr must be a finite number >= 0 (got %r)" % (spec.lr,))
    if not _number(spec.lam) or not 0 <= spec.lam < 1:
        raise ValueError("lam must be a number in [0, 1) (got %r)" % (spec.lam,))
    if not _number(spec.eps) or not math.isfinite(spec.eps) or spec.eps <= 0:
        raise ValueError("eps must be a finite number > 0 (got %r)" % (spec.eps,))
    if spec.rule not in RULES:
        raise ValueError("rule must be one of %s (got %r)" % (", ".join(RULES), spec.rule))
    for name in ("batch_size", "num_steps"):
        if not _whole(getattr(spec, name)) or getattr(spec, name) < 1:
            raise ValueError("%s must be an integer >= 1 (got %r)" % (name, getattr(spec, name)))
    if spec.rule == "rms" and stats is None:
        raise ValueError("rule 'rms' needs gradient statistics (gradient_stats)")
    if stats is not None and cfg is not None:
        check_stats(cfg, stats, n_out)
    return spec


def check_stats(cfg, stats, n_out=None):
    """ValueError unless ``stats`` is a dump-shaped dict of exactly the model's tensors, finite, >= 0 and not zero everywhere"""
    want = {}                                          # key -> shape, or the list of a block list's shapes
    for key, idx, shape, _fan in _train.weight_shapes(cfg, n_out):
        if idx is None:
            want[key] = tuple(shape)
        else:
            want.setdefault(key, []).append(tuple(shape))
    if not isinstance(stats, dict) or sorted(stats) != sorted(want):
        raise ValueError("the statistics hold the tensors %s, the model has %s" % (sorted(stats) if isinstance(stats, dict) else stats,
                                                                                sorted(want)))
    total = 0.0
    for key, shape in want.items():
        have = [tuple(np.shape(a)) for a in stats[key]] if isinstance(shape, list) else tuple(np.shape(stats[key]))
        if have != shape:
            raise ValueError("the statistics of tensor %s have shape %s, the model needs %s" % (key, have, shape))
        for a in (stats[key] if isinstance(shape, list) else [stats[key]]):
            a = np.asarray(a, dtype=np.float64)
            if not np.isfinite(a).all() or (a < 0).any():
                raise ValueError("the statistics of tensor %s are not all finite and >= 0" % key)
            total += float(a.sum())
    if not total > 0:
        raise ValueError("the statistics are zero everywhere: mean(RMS) has to be > 0")


def mean_rms(stats):
    """mean(RMS) over every parameter of a dump-shaped dict, in float64"""
    arrays = [np.asarray(a, dtype=np.float64) for _k, _i, a in _train._items(stats)]
    return float(sum(a.sum() for a in arrays) / sum(a.size for a in arrays))


def _refuse_untied(cfg):
    if not cfg.get("share_embedding", True):
        raise NotImplementedError("share_embedding=False (an untied projection UM) is not built")


class _DynEvalMixin:
    def _take_spec(self, cfg, weights, spec, stats):
        _refuse_untied(cfg)
        self.spec = check_spec(spec, cfg, stats, np.asarray(weights["b2"]).shape[0])
        self._collecting = False

    def set_rates(self, lr, lam):
        """another lr and lam for the chunks to come (:func:`tune` walks its grid on one stepper)"""
        self.spec = check_spec(self.spec.replace(lr=lr, lam=lam), stats=self.stats)
        self.lr = float(lr)

    def _lam_scale(self):
        """what multiplies RMS (rms) or 1 (sgd) in the decay coefficient"""
        return float(self.spec.lam) / self.stats_mean if self.spec.rule == "rms" else float(self.spec.lam)


class DynEvalReferenceStepper(_DynEvalMixin, _train.ReferenceStepper):
    """The dynamic-evaluation step in numpy float64 (module docstring): ``train.ReferenceStepper`` on the plain ``ce`` without dropout,
    its update replaced.  ``stats``: a dump-shaped dict of RMS tensors (:func:`gradient_stats`)."""

    def __init__(self, cfg, weights, spec, stats=None):
        self._take_spec(cfg, weights, spec, stats)
        self.stats = stats
        self.rms = None if stats is None else _train._map(stats, lambda a: np.array(a, dtype=np.float64))
        self.stats_mean = None if stats is None else mean_rms(stats)
        _train.ReferenceStepper.__init__(self, cfg, weights, spec.batch_size, spec.num_steps, lr=spec.lr, dropout=1.0, norm_weight=0.0)

    def load_weights(self, weights):
        _train.ReferenceStepper.load_weights(self, weights)
        self.w0 = _train._map(self.w, np.copy)

    def restore(self):
        """theta <- theta0"""
        self.w = _train._map(self.w0, np.copy)

    def begin_stats(self):
        self._collecting, self._ms = True, _train._map(self.w, np.zeros_like)

    def end_stats(self, n_chunks):
        self._collecting = False
        return _train._map(self._ms, lambda a: np.sqrt(a / n_chunks).astype(np.float32))

    def _one(self, w, g, w0, rms):
        s = self.spec
        if s.rule == "sgd":
            return w - s.lr * g + s.lam * (w0 - w)
        return w - s.lr * g / (rms + s.eps) + np.minimum(self._lam_scale() * rms, 1.0) * (w0 - w)

    def _update(self, g):
        self.t += 1
        for key, idx, a in list(_train._items(self.w)):
            if idx is None:
                if self._collecting:
                    self._ms[key] = self._ms[key] + g[key] * g[key]
                else:
                    self.w[key] = self._one(a, g[key], self.w0[key], None if self.rms is None else self.rms[key])
            elif self._collecting:
                self._ms[key][idx] = self._ms[key][idx] + g[key][idx] * g[key][idx]
            else:
                self.w[key][idx] = self._one(a, g[key][idx], self.w0[key][idx], None if self.rms is None else self.rms[key][idx])


class DynEvalDeviceStepper(_DynEvalMixin, _train.DeviceStepper):
    """The dynamic-evaluation step on the GPU: ``train.DeviceStepper`` with its Adam launch replaced by ``dyneval_update`` and its
    few-tile, long-contraction products routed through ``train_gemm_splitk``.  theta0 and RMS live in the two flat buffers the trainer
    keeps Adam's moments in (``M``, ``Vv``): no step here reads a moment.  ``split_kc`` (a multiple of 16), ``split_max_tiles`` (0:
    every product is the trainer's launch): the routing's two constants."""

    def __init__(self, cfg, weights, spec, stats=None, device=None, chunk_bytes=None, split_kc=None, split_max_tiles=None):
        self._take_spec(cfg, weights, spec, stats)
        self.split_kc = SPLIT_KC if split_kc is None else int(split_kc)
        self.split_max_tiles = SPLIT_MAX_TILES if split_max_tiles is None else int(split_max_tiles)
        if self.split_kc < 16 or self.split_kc % 16 or self.split_max_tiles < 0:
            raise ValueError("split_kc must be a positive multiple of 16 and split_max_tiles >= 0 (got %r, %r)" % (split_kc, split_max_tiles))
        self.stats, self.stats_mean, self._ms = None, None, None
        _train.DeviceStepper.__init__(self, cfg, weights, spec.batch_size, spec.num_steps, lr=spec.lr, dropout=1.0, norm_weight=0.0,
                                      device=device, chunk_bytes=chunk_bytes)
        self.n_real = sum(n for _k, _i, _s, _o, n in self.layout)
        with self.torch.cuda.device(self.dev):
            self.part = self.torch.zeros(0, device=self.dev)               # the splits' tiles; grown to the largest product met
            self.partial = self.torch.zeros(4096, device=self.dev, dtype=self.torch.float64)
            self.mean = self.torch.zeros(1, device=self.dev, dtype=self.torch.float64)
        if stats is not None:
            self.set_stats(stats)

    W0 = property(lambda self: self.M)
    RMS = property(lambda self: self.Vv)

    def load_weights(self, weights):
        _train.DeviceStepper.load_weights(self, weights)
        self.W0.copy_(self.W)

    def restore(self):
        """theta <- theta0: one device copy; a flag word raised by a chunk whose loss was not finite is lowered"""
        self.W.copy_(self.W0)
        self.flag.zero_()

    def _flat(self, tensors):
        flat = np.zeros(self.n_flat, dtype=np.float32)
        for key, idx, shape, off, n in self.layout:
            if key in ("HM", "IM", "b"):
                a = np.concatenate([np.asarray(tensors[key + gname], dtype=np.float32) for gname in _train.GATES], axis=-1)
            else:
                a = np.asarray(tensors[key] if idx is None else tensors[key][idx], dtype=np.float32)
            flat[off:off + n] = a.reshape(-1)
        return flat

    def set_stats(self, stats):
        check_stats(self.cfg, stats, self.d["V"])
        self.stats, self.stats_mean = stats, mean_rms(stats)
        self.RMS.copy_(self.torch.from_numpy(self._flat(stats)))

    def begin_stats(self):
        with self.torch.cuda.device(self.dev):
            self._ms = self.torch.zeros(self.n_flat, device=self.dev)
        self._collecting = True

    def end_stats(self, n_chunks):
        """-> the RMS dict (one read-back); ``device_mean``: mean(RMS) as the device formed it"""
        with self.torch.cuda.device(self.dev):
            rms = self.torch.zeros(self.n_flat, device=self.dev)
            self.ops.dyneval_rms(self._ms, self.n_flat, 1.0 / n_chunks, rms, self.n_real, self.partial, self.mean)
        self._collecting, self._ms = False, None
        out = self._split(rms.cpu().numpy())
        self.device_mean = float(self.mean.item())
        return out

    def _update(self):
        self.t += 1
        if self._collecting:
            self.ops.dyneval_sqacc(self._ms, self.G, self.n_flat, self.flag)
            self._mark("statistics")
            return
        s = self.spec
        self.ops.dyneval_update(self.W, self.G, self.W0, self.RMS if s.rule == "rms" else None, self.n_flat, float(s.lr), self._lam_scale(),
                                float(s.eps), self.flag)
        self._mark("update")

    def _gemm(self, A, sam, sak, B, sbk, sbn, C, ldc, M, N, K, accumulate, bias):
        kc = self.split_kc
        if -(-M // 64) * -(-N // 64) > self.split_max_tiles or K < 2 * kc:
            return self.ops.train_gemm(A, sam, sak, B, sbk, sbn, C, ldc, M, N, K, accumulate, bias)
        need = -(-K // kc) * M * N
        if self.part.numel() < need:
            self.part = self.torch.zeros(need, device=self.dev)
        self.ops.train_gemm_splitk(A, sam, sak, B, sbk, sbn, C, ldc, M, N, K, accumulate, bias, kc, self.part)


# ------------------------------------------------------------------------------------------------- the drivers
def _chunks(stream, batch_size, num_steps):
    from .score import stream_layout
    x, y = stream_layout(stream, batch_size, num_steps)
    for i in range(x.shape[1] // num_steps):
        cols = slice(i * num_steps, (i + 1) * num_steps)
        yield x[:, cols], y[:, cols]


def gradient_stats(stepper, stream, n_chunks):
    """The RMS statistics of the rms rule: ``n_chunks`` backward passes over the first chunks of ``stream`` at the stepper's weights,
    the state carried from the zero state, no update -> a dump-shaped dict of float32 RMS tensors.  On the device the sums of squares
    stay there; what comes back, once at the end, is the RMS buffer.  The stepper's state is zero again afterwards."""
    if not _whole(n_chunks) or n_chunks < 1:
        raise ValueError("n_chunks must be an integer >= 1 (got %r)" % (n_chunks,))
    batches = []
    for xy in _chunks(stream, stepper.B, stepper.T):
        batches.append(xy)
        if len(batches) == n_chunks:
            break
    if len(batches) < n_chunks:
        raise ValueError("the stream has %d chunks of %d x %d, the statistics ask for %d" % (len(batches), stepper.B, stepper.T, n_chunks))
    stepper.reset_state()
    stepper.begin_stats()
    try:
        for x, y in batches:
            stepper.step_async(x, y, True)
    finally:
        out = stepper.end_stats(n_chunks)
    stepper.losses()                                   # NonFiniteLoss where a chunk's loss was not finite
    stepper.reset_state()
    return out


def run_stream(stepper, stream):
    """One dynamic pass over ``stream`` from the zero state and the stepper's current weights -> (perplexity, total nll, n tokens);
    the chunks' ``ce`` come back once, at the end"""
    stepper.reset_state()
    for x, y in _chunks(stream, stepper.B, stepper.T):
        stepper.step_async(x, y, True)
    ce = stepper.losses()
    per = stepper.B * stepper.T
    total, n_tok = float(np.sum(ce) * per), int(len(ce) * per)
    return float(np.exp(total / n_tok)), total, n_tok


def _load(experiment_id, spec, stats, root, stepper, comp):
    """the checks that need no file, the configuration, the checks that need it, the weights, the stepper -- in that order"""
    check_spec(spec, stats=stats)
    if comp:
        raise ValueError("dynamic evaluation runs on the uncompressed weights (comp = %r)" % (comp,))
    if not (stepper is None or stepper == "reference" or callable(stepper)):
        raise ValueError("stepper is None, 'reference' or a callable (got %r)" % (stepper,))
    if root:
        _config.set_root(root)
    cfg = _config.load_config_dict(experiment_id)
    _refuse_untied(cfg)
    if cfg.get("class_based"):
        raise ValueError("class_based models are not built")
    if stats is not None:
        n_out = np.asarray(stats["b2"]).shape[0] if isinstance(stats, dict) and "b2" in stats else None
        check_stats(cfg, stats, n_out)
    weights = _weights.load_weights(experiment_id, 0, cfg)
    if stepper is None:
        from . import _lib
        _lib.require_gpu()
        return DynEvalDeviceStepper(cfg, weights, spec, stats)
    if stepper == "reference":
        return DynEvalReferenceStepper(cfg, weights, spec, stats)
    return stepper(cfg, weights, spec, stats)


def dynamic_perplexity(experiment_id, stream, spec, stats=None, root=None, stepper=None, comp=0):
    """The dynamically evaluated perplexity of the id stream ``stream`` under experiment ``experiment_id``: -> (perplexity, total nll,
    number of tokens) over the chunks of ``score.stream_layout`` at ``spec.batch_size`` x ``spec.num_steps``.  ``stats``: the RMS dict
    of :func:`gradient_stats` (rule "rms").  ``stepper``: None = :class:`DynEvalDeviceStepper`, ``"reference"`` =
    :class:`DynEvalReferenceStepper`, or a callable ``(cfg, weights, spec, stats) -> stepper``.  ValueError before any file is read
    for a bad spec, rms without statistics, ``comp`` != 0 and an unknown stepper; for statistics that are not the model's before the
    weights are read and anything is launched."""
    return run_stream(_load(experiment_id, spec, stats, root, stepper, comp), stream)


def experiment_stats(experiment_id, stream, n_chunks, batch_size=1, num_steps=5, root=None, stepper=None):
    """:func:`gradient_stats` of experiment ``experiment_id`` at its loaded weights over the first ``n_chunks`` chunks of ``stream``
    (the training text) -- all of them where the stream is shorter"""
    from .score import stream_layout
    have = stream_layout(stream, batch_size, num_steps)[0].shape[1] // num_steps
    st = _load(experiment_id, DynEvalSpec(0.0, batch_size=batch_size, num_steps=num_steps), None, root, stepper, 0)
    return gradient_stats(st, stream, min(int(n_chunks), have))


def tune(experiment_id, stream, lrs, lams, rule="sgd", eps=1e-3, batch_size=1, num_steps=5, stats=None, root=None, stepper=None):
    """Every (lr, lam) of the grid on ``stream`` (held-out text), each a pass of its own from theta0 and the zero state.
    -> (grid float64 [len(lrs), len(lams)] of perplexities, inf where a pass met a loss that is not finite; (best lr, best lam))"""
    lrs, lams = [float(v) for v in lrs], [float(v) for v in lams]
    if not lrs or not lams:
        raise ValueError("the grid is empty")
    for lr in lrs:
        for lam in lams:
            check_spec(DynEvalSpec(lr, lam, rule, eps, batch_size, num_steps), stats=stats)
    st = _load(experiment_id, DynEvalSpec(lrs[0], lams[0], rule, eps, batch_size, num_steps), stats, root, stepper, 0)
    grid = np.full((len(lrs), len(lams)), np.inf)
    for i, lr in enumerate(lrs):
        for j, lam in enumerate(lams):
            st.restore()
            st.set_rates(lr, lam)
            try:
                grid[i, j] = run_stream(st, stream)[0]
            except _train.NonFiniteLoss:
                pass
    if not np.isfinite(grid).any():
        raise _train.NonFiniteLoss(0)
    i, j = np.unravel_index(int(np.argmin(grid)), grid.shape)
    return grid, (lrs[i], lams[j])
