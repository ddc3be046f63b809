"""Retraining the codebooks of a k-means compressed model on the device: ``finetune_experiment``, ``python -m jlm_amd.finetune``.

The second half of Deep Compression's quantisation (Han, Mao, Dally 2016, section 3): after the clustering (``jlm_amd.compress``) the
codes stay fixed and the shared centroids are trained.  The reference's train/comp.py stops after the clustering.

The step.  A model is ``name -> (code uint8, codebook float32 [K, 1])`` with K = 2^bit for every tensor -- what
``weights.load_codes`` returns.  The weights of a step are ``W[name] = take(codebook[name], code[name])``; the forward and backward
passes are those of ``jlm_amd.train``, unchanged; the gradient of codebook entry j is the sum of ``dW`` over the elements whose code is
j; Adam (TensorFlow's form, ``train.adam_lr_t``, the step counter that also keys the dropout masks) runs on the codebooks only, one
``(m, v)`` pair per entry.  A code that no element carries has gradient 0 and its entry stays where it is (m = v = 0 give a zero
update).  After every step each weight is again exactly ``take(codebook, code)``.

:class:`CodebookReferenceStepper` is that step in numpy float64 on top of ``train.ReferenceStepper``; :class:`CodebookDeviceStepper`
sits on ``train.DeviceStepper`` and replaces its Adam launch by ``train_codebook_grad``, ``train_adam`` over the codebook buffer and
``train_expand_codes`` (csrc/jlm_train.hip).  Both replace only ``_update`` and the weight accessors.

There is no CPU fallback for real fine-tuning: ``finetune_experiment`` needs the GPU, like the rest of the package.
"""
import argparse
import os
import pickle
import shutil

import numpy as np

from . import config as _config
from . import train as _train
from . import weights as _weights
from .compress import write_compressed
from .train import GATES

CODEBOOK_CHUNK = 4096                # JLM_CODEBOOK_CHUNK (include/jlm_hip.h)
OVERRIDES = ("lr", "max_epochs", "early_stopping", "batch_size", "num_steps", "dropout", "tf_random_seed")


# ------------------------------------------------------------------------------------------------- the model as codes and codebooks
def tensor_names(cfg, n_out=None):
    """the dump's tensor names in ``train.weight_shapes`` order: a tensor's index in this list is its place in the codebook buffer"""
    return [key for key, _idx, _shape, _fan in _train.weight_shapes(cfg, n_out)]


def check_codes(cfg, codes, books, n_out=None):
    """ValueError unless ``codes`` / ``books`` hold exactly the tensors of ``cfg``, every code uint8 of the tensor's shape and every
    codebook of one length K = 2^bit.  -> K"""
    if cfg.get("D_softmax"):
        raise ValueError("a D_softmax block list cannot be fine-tuned (compress_experiment cannot compress one either)")
    shapes = {key: tuple(shape) for key, _idx, shape, _fan in _train.weight_shapes(cfg, n_out)}
    if sorted(codes) != sorted(shapes) or sorted(books) != sorted(shapes):
        raise ValueError("the compressed model holds the tensors %s, the configuration needs %s" % (sorted(codes), sorted(shapes)))
    sizes = sorted({int(np.asarray(books[k]).size) for k in shapes})
    K = sizes[0]
    if len(sizes) != 1 or K < 2 or K > 256 or K & (K - 1):
        raise ValueError("every codebook must have the same length 2^bit, 1 <= bit <= 8 (got the lengths %s)" % sizes)
    for k, shape in shapes.items():
        c = np.asarray(codes[k])
        if c.dtype != np.uint8 or tuple(c.shape) != shape:
            raise ValueError("the code of tensor %s is %s %s, the model needs uint8 %s" % (k, c.dtype, tuple(c.shape), shape))
        if int(c.max()) >= K:
            raise ValueError("the code of tensor %s reaches %d, its codebook has %d entries" % (k, int(c.max()), K))
    return K


def decode(codes, books):
    """name -> take(codebook, code), float32 (train/comp.py:70)"""
    return {k: np.take(np.asarray(books[k], dtype=np.float32).reshape(-1), np.asarray(codes[k])) for k in codes}


def books_from_weights(codes, books, w):
    """What ``load_weights`` does with a decoded dict ``w``: entry j of every codebook from the elements that carry code j; an entry
    without elements keeps its value.  ValueError where two elements of one code differ or a shape is wrong.  ``books``: name -> [K]
    or [K, 1] of any float type; -> name -> the same shape and type."""
    out = {}
    for k, code in codes.items():
        if k not in w:
            raise ValueError("tensor %s is missing" % k)
        a = np.asarray(w[k])
        if a.shape != code.shape:
            raise ValueError("tensor %s has shape %s, the model needs %s" % (k, a.shape, code.shape))
        book = np.array(books[k])
        flat = book.reshape(-1)
        c, v = code.reshape(-1), a.reshape(-1).astype(flat.dtype)
        used, first = np.unique(c, return_index=True)
        flat[used] = v[first]
        if not np.array_equal(flat[c], v):
            raise ValueError("tensor %s is not a codebook's image: two elements of one code differ" % k)
        out[k] = book
    return out


def build_groups(layout, names, codes, K, n_flat, chunk=CODEBOOK_CHUNK):
    """The device's view of the codes, built once per stepper (host, numpy).  ``layout``: ``DeviceStepper.layout`` -- the flat parameter
    buffer holds the four gate matrices side by side ([H, 4H], [E, 4H], [4H]), so columns [k H', (k + 1) H') of "HM" carry the codes of
    ``HM`` + "ifog"[k]; ``names``: :func:`tensor_names`.
    -> gid int32 [n_flat]: tensor index * K + code, -1 on the padding between tensors;
       order int32: the flat offsets of all coded elements sorted by (gid, offset);
       chunks int32 [n_chunks, 3] = (group, begin, length): every group's run of ``order`` in pieces of at most ``chunk``."""
    index = {k: t for t, k in enumerate(names)}
    gid = np.full(int(n_flat), -1, dtype=np.int32)
    for key, idx, shape, off, n in layout:
        if idx is not None:
            raise ValueError("a D_softmax block list cannot be fine-tuned")
        if key in ("HM", "IM", "b"):
            a = np.concatenate([index[key + g] * K + np.asarray(codes[key + g]).astype(np.int32) for g in GATES], axis=-1)
        else:
            a = index[key] * K + np.asarray(codes[key]).astype(np.int32)
        if a.shape != tuple(shape):
            raise ValueError("the code of tensor %s has shape %s, the model needs %s" % (key, a.shape, tuple(shape)))
        gid[off:off + n] = a.reshape(-1)
    coded = np.nonzero(gid >= 0)[0]                                  # ascending offsets: a stable sort by gid keeps them so
    order = coded[np.argsort(gid[coded], kind="stable")].astype(np.int32)
    counts = np.bincount(gid[coded], minlength=len(names) * K).astype(np.int64)
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
    per = -(-counts // chunk)                                        # chunks per group; 0 for an empty one
    group = np.repeat(np.arange(len(counts)), per)
    within = np.arange(int(per.sum())) - np.repeat(np.concatenate([[0], np.cumsum(per)[:-1]]), per)
    begin = starts[group] + within * chunk
    length = np.minimum(chunk, starts[group] + counts[group] - begin)
    chunks = np.stack([group, begin, length], axis=1).astype(np.int32).reshape(-1, 3)
    return gid, order, chunks


# ------------------------------------------------------------------------------------------------- the two steppers
class _CodebookMixin:
    def _take_codes(self, cfg, codes, books):
        self._codes = {k: np.ascontiguousarray(np.asarray(v)) for k, v in codes.items()}
        n_out = np.asarray(codes["b2"]).shape[0] if "b2" in codes else None
        self.K = check_codes(cfg, self._codes, books, n_out)
        self.names = tensor_names(cfg, n_out)

    def codes(self):
        return {k: v.copy() for k, v in self._codes.items()}


class CodebookReferenceStepper(_CodebookMixin, _train.ReferenceStepper):
    """The fine-tuning step in numpy float64 (module docstring): ``train.ReferenceStepper`` with its update replaced."""

    def __init__(self, cfg, codes, books, batch_size, num_steps, lr=1e-3, dropout=1.0, norm_weight=0.1, seed=0):
        self._take_codes(cfg, codes, books)
        self.book = {k: np.array(books[k], dtype=np.float64).reshape(self.K, 1) for k in self.names}
        self.bm = {k: np.zeros((self.K, 1)) for k in self.names}
        self.bv = {k: np.zeros((self.K, 1)) for k in self.names}
        self._gbook = None
        _train.ReferenceStepper.__init__(self, cfg, decode(self._codes, books), batch_size, num_steps, lr, dropout, norm_weight, seed)

    def _expand(self):
        self.w = {k: np.take(self.book[k].reshape(-1), self._codes[k]) for k in self.names}

    def load_weights(self, weights):
        self.book = books_from_weights(self._codes, self.book, weights)
        self._expand()

    def weights(self):
        return {k: a.astype(np.float32) for k, a in self.w.items()}

    def codebooks(self):
        return {k: b.astype(np.float32) for k, b in self.book.items()}

    def codebook_grads(self):
        """the last training step's codebook gradients: name -> float64 [K, 1]"""
        return self._gbook

    def _update(self, g):
        self.t += 1
        self._gbook = {}
        for k in self.names:
            gb = np.bincount(self._codes[k].reshape(-1), weights=np.asarray(g[k], dtype=np.float64).reshape(-1), minlength=self.K)
            self._gbook[k] = gb.reshape(self.K, 1)
            self.book[k], self.bm[k], self.bv[k] = _train.adam_reference(self.book[k], self._gbook[k], self.bm[k], self.bv[k], self.t, self.lr)
        self._expand()


class CodebookDeviceStepper(_CodebookMixin, _train.DeviceStepper):
    """The fine-tuning step on the GPU: ``train.DeviceStepper`` with its Adam launch replaced by ``train_codebook_grad`` (the
    gradients of the flat parameter buffer summed per code), ``train_adam`` over the codebook buffer and ``train_expand_codes`` (the
    flat parameter buffer written again from the codebooks).  The codebooks live in one float32 buffer, tensor t at t K, padded to a
    multiple of 4, with gradient, m and v buffers of the same length."""

    def __init__(self, cfg, codes, books, batch_size, num_steps, lr=1e-3, dropout=1.0, norm_weight=0.1, seed=0, device=None, chunk_bytes=None):
        self._take_codes(cfg, codes, books)
        self._book0 = {k: np.array(books[k], dtype=np.float32).reshape(self.K, 1) for k in self.names}
        self.gid = None
        _train.DeviceStepper.__init__(self, cfg, decode(self._codes, books), batch_size, num_steps, lr, dropout, norm_weight, seed, device,
                                      chunk_bytes)

    def _tables(self):
        """the device data of section 14, built from the codes when the first weights arrive (the layout exists by then)"""
        torch, K = self.torch, self.K
        gid, order, chunks = build_groups(self.layout, self.names, self._codes, K, self.n_flat)
        self.n_groups, self.n_chunks = len(self.names) * K, len(chunks)
        self.n_book = (self.n_groups + 3) // 4 * 4
        with torch.cuda.device(self.dev):
            self.gid = torch.from_numpy(gid).to(self.dev)
            self.order = torch.from_numpy(order).to(self.dev)
            self.chunks = torch.from_numpy(np.ascontiguousarray(chunks).reshape(-1)).to(self.dev)
            self.partial = torch.zeros(max(1, self.n_chunks), device=self.dev, dtype=torch.float64)
            self.book, self.gbook, self.bm, self.bv = (torch.zeros(self.n_book, device=self.dev) for _ in range(4))
        self._set_books(self._book0)

    def _set_books(self, books):
        flat = np.zeros(self.n_book, dtype=np.float32)
        for t, k in enumerate(self.names):
            flat[t * self.K:(t + 1) * self.K] = np.asarray(books[k], dtype=np.float32).reshape(-1)
        with self.torch.cuda.device(self.dev):
            self.book.copy_(self.torch.from_numpy(flat))
            self.ops.train_expand_codes(self.book, self.gid, self.W, self.n_flat)

    def _books_of(self, buf):
        flat = buf.cpu().numpy()
        return {k: flat[t * self.K:(t + 1) * self.K].reshape(self.K, 1).copy() for t, k in enumerate(self.names)}

    def load_weights(self, weights):
        if self.gid is None:
            self._tables()
        self._set_books(books_from_weights(self._codes, self.codebooks(), weights))

    def codebooks(self):
        return self._books_of(self.book)

    def codebook_grads(self):
        """the last training step's codebook gradients: name -> float32 [K, 1]"""
        return self._books_of(self.gbook)

    def _update(self):
        O = self.ops
        self.t += 1
        O.train_codebook_grad(self.G, self.order, self.chunks, self.n_chunks, self.n_groups, self.partial, self.gbook)
        self._mark("codebook_grad")
        O.train_adam(self.book, self.gbook, self.bm, self.bv, self.n_book, _train.adam_lr_t(self.lr, self.t), self.flag)
        self._mark("adam")
        O.train_expand_codes(self.book, self.gid, self.W, self.n_flat)
        self._mark("expand")


# ------------------------------------------------------------------------------------------------- the driver
def _dump_path(experiment_id, bit, name="lstm_weights_comp_dump.pkl"):
    return os.path.join(_weights.weights_dir(experiment_id), "comp_{}".format(bit), name)


def _has_text_dumps(experiment_id, bit):
    cdir = os.path.dirname(_dump_path(experiment_id, bit))
    return os.path.isdir(cdir) and any(fn.endswith("_code.txt") for fn in os.listdir(cdir))


def finetune_experiment(experiment_id, bit, parameters=None, root=None, log=print, stepper=None, verbose=10):
    """Retrain the codebooks of experiment ``experiment_id`` compressed at ``bit`` bits, and write the result over the compressed
    files when it beats the k-means codebooks on the validation set.
    ``parameters`` may override lr, max_epochs, early_stopping, batch_size, num_steps, dropout and tf_random_seed; everything else is
    the experiment's config.json.  ``stepper``: None = :class:`CodebookDeviceStepper`, ``"reference"`` =
    :class:`CodebookReferenceStepper`, or a callable ``(cfg, codes, books, batch_size, num_steps, lr, dropout, norm_weight, seed) ->
    stepper``.  A save writes what ``compress_experiment`` writes (``compress.write_compressed``); before the first one the k-means
    dump is kept as comp_{bit}/lstm_weights_comp_dump.kmeans.pkl, which a later run does not overwrite.
    ValueError before anything is launched or written: unknown parameters, a D_softmax block list, no (code, codebook) dump for
    that bit, codebooks that are not all of length 2^bit, tensor shapes that do not match the configuration.
    -> dict(kmeans_valid_pp, best_valid_pp, history, test_pp, best_test_pp, saved)"""
    from .data import CharVocab, Vocab
    parameters = dict(parameters or {})
    unknown = sorted(set(parameters) - set(OVERRIDES))
    if unknown:
        raise ValueError("fine-tuning takes the parameters %s (got also: %s)" % (", ".join(OVERRIDES), ", ".join(unknown)))
    is_int = isinstance(bit, (int, np.integer)) and not isinstance(bit, bool)
    if not is_int or not 1 <= bit <= 8:
        raise ValueError("bit must be an integer in [1, 8] (got %r)" % (bit,))
    if root:
        _config.set_root(root)
    cfg = _config.load_config_dict(experiment_id)
    p = _train.check_parameters(dict({k: v for k, v in cfg.items() if k in _train.DEFAULTS}, **parameters))
    if p["D_softmax"]:
        raise ValueError("a D_softmax block list cannot be fine-tuned (compress_experiment cannot compress one either)")
    pairs = _weights.load_codes(experiment_id, bit)
    if not pairs:
        raise ValueError("experiment %s has no (code, codebook) dump for %d bits: run jlm_amd.compress first" % (experiment_id, bit))
    codes = {k: c for k, (c, _b) in pairs.items()}
    books = {k: b for k, (_c, b) in pairs.items()}
    n_out = int(np.asarray(codes["b2"]).shape[0]) if "b2" in codes and np.asarray(codes["b2"]).ndim == 1 else None
    if not p["char_rnn"] and n_out != p["vocab_size"]:
        raise ValueError("the compressed model has %s output words, the configuration's vocab_size is %d" % (n_out, p["vocab_size"]))
    K = check_codes(p, codes, books, n_out)
    if K != 1 << bit:
        raise ValueError("the codebooks of comp_%d have %d entries, not 2^%d" % (bit, K, bit))
    vocab = (CharVocab if p["char_rnn"] else Vocab)(p["vocab_size"])
    if len(vocab) != n_out:
        raise ValueError("the lexicon gives %d words, the compressed model has %d" % (len(vocab), n_out))
    train_data, dev_data, test_data = _train.load_corpus(vocab, p["debug"])
    kw = dict(batch_size=p["batch_size"], num_steps=p["num_steps"], lr=p["lr"], dropout=p["dropout"], norm_weight=p["norm_weight"],
              seed=p["tf_random_seed"])
    if stepper is None:
        import torch
        from . import _lib
        _lib.require_gpu()
        dev = torch.device("cuda", int(p["gpu_id"]) if int(p["gpu_id"]) < torch.cuda.device_count() else torch.cuda.current_device())
        st = CodebookDeviceStepper(p, codes, books, device=dev, **kw)
    elif stepper == "reference":
        st = CodebookReferenceStepper(p, codes, books, **kw)
    else:
        st = stepper(p, codes, books, **kw)
    B, T = int(p["batch_size"]), int(p["num_steps"])
    kmeans_pp = _train.run_epoch(st, dev_data, B, T, False)
    log("Validation perplexity (k-means): {}".format(kmeans_pp))
    start = st.weights()
    saved = []

    def save(_weights_of_the_epoch):
        dump_file, backup = _dump_path(experiment_id, bit), _dump_path(experiment_id, bit, "lstm_weights_comp_dump.kmeans.pkl")
        raw = None
        if os.path.exists(dump_file):
            with open(dump_file, "rb") as f:
                raw = pickle.load(f)
        if not os.path.exists(backup):
            if raw is not None:
                shutil.copyfile(dump_file, backup)
            else:
                os.makedirs(os.path.dirname(backup), exist_ok=True)
                with open(backup, "wb") as f:
                    pickle.dump({k: (codes[k], books[k].reshape(-1, 1)) for k in codes}, f)
        new = st.codebooks()
        order = list(raw) if raw is not None else list(codes)
        dump = {k: (raw[k][0] if raw is not None else codes[k], np.asarray(new[k], dtype=np.float32).reshape(-1, 1)) for k in order}
        write_compressed(experiment_id, bit, dump, _has_text_dumps(experiment_id, bit))
        saved.append(len(saved))

    result = _train.fit(st, train_data, dev_data, test_data, p, log, save, verbose, best_pp=kmeans_pp)
    if not saved:                                   # no epoch beat the k-means codebooks: they are what stays, on disk and here
        st.load_weights(start)
        result["best_test_pp"] = _train.run_epoch(st, test_data, B, T, False)
        log("Test perplexity of the k-means codebooks (no epoch was better): {}".format(result["best_test_pp"]))
    return dict(kmeans_valid_pp=kmeans_pp, best_valid_pp=result["best_valid_pp"], history=result["history"], test_pp=result["test_pp"],
                best_test_pp=result["best_test_pp"], saved=bool(saved))


# ------------------------------------------------------------------------------------------------- command line
def build_parser():
    ap = argparse.ArgumentParser(description="Retrain the codebooks of a k-means compressed experiment on the device (Deep Compression's "
                                             "second half; the reference's train/comp.py stops after the clustering)")
    ap.add_argument("--root", default=None, help="artifact root (default: jlm_amd.config's)")
    ap.add_argument("--experiment", "-e", dest="experiment", default="10", help="which experiment to fine-tune")
    ap.add_argument("--comp", "-c", dest="comp", type=int, required=True, help="the compression's bits (1 .. 8)")
    for key in OVERRIDES:
        ap.add_argument("--" + key, type=type(_train.DEFAULTS[key]), default=None,
                        help="instead of the experiment's config.json (train/train.py parameters[%r])" % key)
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    over = {k: getattr(args, k) for k in OVERRIDES if getattr(args, k) is not None}
    r = finetune_experiment(args.experiment, args.comp, over, root=args.root)
    print("perplexity: k-means {:.4f} (validation)  fine-tuned {:.4f} (validation, {})  test {:.4f}".format(
        r["kmeans_valid_pp"], r["best_valid_pp"], "saved" if r["saved"] else "not saved: the k-means codebooks stay", r["best_test_pp"]))
    return r


if __name__ == "__main__":
    main()
