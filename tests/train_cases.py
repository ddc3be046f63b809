"""Shared helpers of tests/test_train_cpu.py, tests/test_gpu_train.py and tests/test_gpu_train_shapes.py: the Markov corpus, the model
configurations (the odd-sized one among them), and the training graph restated in torch (autograd) -- the test's own words for
reference train/model.py, independent of jlm_amd.train's backward pass."""
import os

import numpy as np

from jlm_amd import synth

MARKOV_V = 600
MARKOV_P = (0.55, 0.25, 0.15, 0.05)


def markov_stream(n, seed=3, V=MARKOV_V):
    """n ids of the walk: nxt = RandomState(seed).randint(1, V, (V, 4)); from id 1, each step to nxt[cur, k], k ~ MARKOV_P"""
    rng = np.random.RandomState(seed)
    nxt = rng.randint(1, V, (V, 4))
    ks = rng.choice(4, size=n, p=MARKOV_P)
    out = np.empty(n, dtype=np.int64)
    cur = 1
    for i in range(n):
        cur = nxt[cur, ks[i]]
        out[i] = cur
    return out


def unigram_perplexity(train, dev, V=MARKOV_V):
    """add-one unigram perplexity of ``dev`` under the counts of ``train``"""
    cnt = np.bincount(train, minlength=V).astype(np.float64)
    logp = np.log((cnt + 1.0) / (cnt.sum() + V))
    return float(np.exp(-logp[dev].mean()))


def write_markov_corpus(root, n_train=48032, n_dev=3232, n_test=3232, seed=3, V=MARKOV_V):
    """The walk written as data/train.txt, dev.txt, test.txt through a synthetic lexicon of V - 1 words (id 0 is <unk>, id 1 <eos>): a
    line ends where the walk visits id 1 (the encoder appends <eos>); a visit to 1 right after another cannot be written as a line and is
    dropped.  -> (train, dev, test) id streams AS THE FILES ENCODE (what the trainer reads)"""
    from jlm_amd.data import Vocab
    from jlm_amd.perplexity import encode_lines
    lexicon, _rd = synth.write_lexicon(root, V, oov_frac=0.0, alphabet=12)      # 12 kana: a dense lattice for the decode check
    vocab = Vocab(V, lexicon)
    walk = markov_stream(n_train + n_dev + n_test, seed, V)
    cuts = {"train.txt": walk[:n_train], "dev.txt": walk[n_train:n_train + n_dev], "test.txt": walk[n_train + n_dev:]}
    out = []
    for name, ids in cuts.items():
        lines, cur = [], []
        for i in ids:
            if i == 1:
                if cur:
                    lines.append(" ".join(cur))
                cur = []
            else:
                cur.append(vocab.i2w[int(i)])
        if cur:
            lines.append(" ".join(cur))
        with open(os.path.join(root, "data", name), "w", encoding="utf-8") as f:
            f.write("\n".join(lines) + "\n")
        sents, n_unk = encode_lines(lines, vocab)
        assert n_unk == 0
        out.append(np.array([i for s in sents for i in s], dtype=np.int32))
    return out


def small_cfg(mode, V=600, H=64, E=32, self_norm=False, char_rnn=False, segs=None):
    if segs is None:
        segs = [(E, 0, V // 4), (E // 2, V // 4, (3 * V) // 5), (E // 4, (3 * V) // 5, None)]
    return synth.make_config(V, H, E, mode, segs, self_norm, char_rnn)


def driver_parameters(mode, self_norm=False, dropout=0.9, V=MARKOV_V, **over):
    """the parameters of the driver runs (ISSUE item 5): H = 64, E = 32, B = 32, T = 10, lr = 5e-3, 4 epochs"""
    p = dict(vocab_size=V, hidden_size=64, embed_size=32, batch_size=32, num_steps=10, lr=5e-3, max_epochs=4, early_stopping=1,
             dropout=dropout, tf_random_seed=101, share_embedding=True, D_softmax=mode == "dsoftmax", V_table=mode == "vtable",
             embedding_seg=[(32, 0, 150), (16, 150, 360), (8, 360, None)], self_norm=self_norm, norm_weight=0.1, gpu_id=0)
    p.update(over)
    return p


def torch_grads(cfg, weights, x, y, h0, c0, mask_in, mask_out, norm_weight, dtype=None):
    """One step's loss and gradients by torch autograd.  weights: dump-shaped dict; x, y [B, T]; h0, c0 [B, H]; mask_in [T B, E] /
    mask_out [T B, H] in time-major row order (row = t B + b).  -> (ce, dict of gradients, dump-shaped, numpy)"""
    import torch
    dtype = dtype or torch.float64
    B, T = x.shape
    V = np.asarray(weights["b2"]).shape[0]
    leaves = {}

    def leaf(key, idx=None):
        a = weights[key] if idx is None else weights[key][idx]
        t = torch.tensor(np.asarray(a, dtype=np.float64), dtype=dtype, requires_grad=True)
        leaves[(key, idx)] = t
        return t

    segs = [(s[0], s[1], V if s[2] is None else s[2]) for s in cfg["embedding_seg"]]
    if cfg["V_table"]:
        parts = [leaf("LM0")]
        for i in range(1, len(segs)):
            parts.append(torch.matmul(leaf("LM%d" % i), leaf("VT%d" % i)))
        embedding = torch.cat(parts, dim=0)
    elif cfg["D_softmax"]:
        width = sum(s[0] for s in segs)
        rows, c0_ = [], 0
        for i, (size, s, e) in enumerate(segs):
            blk = leaf("LM", i)
            rows.append(torch.cat([torch.zeros(e - s, c0_, dtype=dtype), blk, torch.zeros(e - s, width - c0_ - size, dtype=dtype)], dim=1))
            c0_ += size
        embedding = torch.cat(rows, dim=0)
    else:
        embedding = leaf("LM")
    xs = torch.as_tensor(np.asarray(x, dtype=np.int64))
    inputs = embedding[xs]                                                  # [B, T, E]
    m_in = torch.tensor(np.asarray(mask_in, dtype=np.float64), dtype=dtype).reshape(T, B, -1)
    m_out = torch.tensor(np.asarray(mask_out, dtype=np.float64), dtype=dtype).reshape(T, B, -1)
    Hm = {g: leaf("HM" + g) for g in "ifog"}
    Im = {g: leaf("IM" + g) for g in "ifog"}
    bs = {g: leaf("b" + g) for g in "ifog"}
    state = torch.tensor(np.asarray(h0, dtype=np.float64), dtype=dtype)
    cell = torch.tensor(np.asarray(c0, dtype=np.float64), dtype=dtype)
    rnn_outputs = []
    for t in range(T):
        cur = inputs[:, t, :] * m_in[t]
        pre = {g: torch.matmul(state, Hm[g]) + torch.matmul(cur, Im[g]) + bs[g] for g in "ifog"}
        i, f, o, g = torch.sigmoid(pre["i"]), torch.sigmoid(pre["f"]), torch.sigmoid(pre["o"]), torch.tanh(pre["g"])
        cell = cell * f + g * i
        state = torch.tanh(cell) * o
        rnn_outputs.append(state * m_out[t])
    U = torch.matmul(leaf("PM"), embedding.t())
    b2 = leaf("b2")
    outputs = [torch.matmul(o, U) + b2 for o in rnn_outputs]
    output = torch.cat(outputs, 1).reshape(-1, V)                           # row b T + t
    labels = torch.as_tensor(np.asarray(y, dtype=np.int64)).reshape(-1)
    lse = torch.logsumexp(output, dim=1)
    ce = (lse - output[torch.arange(output.shape[0]), labels]).mean()
    loss = ce
    if norm_weight:
        loss = loss + norm_weight * (lse * lse).mean()
    loss.backward()
    grads = {}
    for (key, idx), t in leaves.items():
        gnp = t.grad.detach().to(torch.float64).numpy()
        if idx is None:
            grads[key] = gnp
        else:
            grads.setdefault(key, {})[idx] = gnp
    for key in list(grads):
        if isinstance(grads[key], dict):
            grads[key] = [grads[key][i] for i in sorted(grads[key])]
    return float(ce.detach()), grads, (state.detach().to(torch.float64).numpy(), cell.detach().to(torch.float64).numpy())


def flat_items(w):
    for k in sorted(w):
        if isinstance(w[k], list):
            for i, a in enumerate(w[k]):
                yield "%s[%d]" % (k, i), np.asarray(a)
        else:
            yield k, np.asarray(w[k])


# ---- the odd-sized model of tests/test_gpu_train_shapes.py: no size a multiple of 4, so the flat parameter buffer has padding
ODD_V, ODD_H = 157, 23
ODD_SEGS = [(19, 0, 40), (9, 40, 93), (5, 93, None)]


def odd_cfg(mode, self_norm=True):
    """V = 157, H = 23, segment widths 19 / 9 / 5: E = 19 (tied, V_table) or 33 (D_softmax).  b2, PM, LM, LM1, VT1 and VT2 have sizes
    that are no multiple of 4, so the device's flat buffer pads them."""
    return small_cfg(mode, ODD_V, ODD_H, 19, self_norm, segs=ODD_SEGS)


def batch(V, B, Tn, seed):
    rng = np.random.RandomState(seed)
    return rng.randint(0, V, (B, Tn)), rng.randint(0, V, (B, Tn))


def carried_state(B, H, seed):
    """a non-zero h, c ~ N(0, 0.3): with it no gradient tensor of a step is identically zero"""
    rng = np.random.RandomState(seed)
    return rng.normal(0, 0.3, (B, H)).astype(np.float32), rng.normal(0, 0.3, (B, H)).astype(np.float32)


def padding_mask(layout, n_flat):
    """bool [n_flat]: True on the words of DeviceStepper's flat buffer that belong to no tensor"""
    pad = np.ones(int(n_flat), dtype=bool)
    for _key, _idx, _shape, off, n in layout:
        pad[off:off + n] = False
    return pad


def worst_relative(got, want):
    """per tensor: the largest deviation in units of the reference tensor's largest magnitude (dump-shaped dicts)"""
    want, got = dict(flat_items(want)), dict(flat_items(got))
    assert sorted(want) == sorted(got)
    out = {}
    for k in want:
        scale = np.abs(want[k]).max()
        assert scale > 0, k                                  # an all-zero reference tensor would make its bar vacuous
        out[k] = float(np.abs(got[k] - want[k]).max() / scale)
    return out


# ---- fine-tuning: the quantiser and the image check of tests/test_gpu_finetune.py and tests/test_gpu_train_shapes.py
def grid_quantise(v, K):
    """a tensor on K evenly spaced levels between its extremes (Glorot weights are uniform, so this is close to what k-means finds, at
    no cost): -> (code uint8, codebook float32 [K, 1]).  At K = 256 the 64-element biases leave most codes empty."""
    book = np.linspace(float(v.min()), float(v.max()), K).astype(np.float32)
    code = np.rint((v.astype(np.float64) - float(v.min())) / (float(v.max()) - float(v.min())) * (K - 1)).astype(np.uint8)
    return code, book.reshape(K, 1)


def codebook_image(st):
    """every weight of a fine-tuning stepper is exactly take(codebook, code), float32"""
    w, b, c = st.weights(), st.codebooks(), st.codes()
    for k in c:
        assert w[k].dtype == np.float32 and w[k].tobytes() == np.take(b[k], c[k]).tobytes(), k
