"""Row formats of the vocabulary normaliser: the rules that say which segments take mixed rows and with which scales, and
the record of that choice (:class:`MixedRows`).  Pure host arithmetic: nothing here launches or keeps device state
(a record points at the packed tensors it was built with, no more).  Layouts: include/jlm_hip.h."""
import collections
import dataclasses

import numpy as np

LOG2E = 1.4426950408889634

# (k + 2 -> 32-k blocks, 16-k f16 steps) with inlined mixed-row bodies: k = 200, 100, 50 (csrc/jlm_mixed.hip MX_KERNEL_DSOFTMAX; the
# first two also in csrc/jlm_split.hip vocab_lse_hybrid_kernel, beside split-row bodies for other short segments)
MIXED_SHAPES = ((7, 13), (4, 7), (2, 4))


def pow2_below(limit, value):
    """the largest e (within +-40) with value 2^e <= limit; 0 for a value without a size"""
    if not (value > 0.0) or not np.isfinite(value):
        return 0
    return int(np.clip(np.floor(np.log2(limit / value)), -40, 40))


def split_bias_correction(t_scale):
    """What a bias must be multiplied by before it is packed into the bias column of split rows.  The normaliser kernels feed that
    column the constant 1.0 like any T value (csrc/jlm_split.hip): scaled by f32(t_scale log2 e) and split into f16 hi + lo.  Those 22
    bits hold log2(e) (1 + 6.9e-8) -- the same relative error on every word's bias, on every row: with a unigram-like bias of -7 under
    the model's distribution that is -4.8e-7 on every log-normaliser, the same sign on every token (tests/test_gpu_score_budget.py
    measured it; it summed to three quarters of a 35-word sentence's score error).  The correction is the exact constant over the held
    one; the loader applies it in float64 and splits that product into the column's hi / lo itself, so what remains is each word's
    own rounding to 22 bits."""
    x = np.float32(np.float32(t_scale) * np.float32(LOG2E))
    hi = np.float16(x)
    lo = np.float16(x - np.float32(hi))
    return float(t_scale) * LOG2E / (float(hi) + float(lo))


def mixed_shape(k):
    """(32-k blocks, 16-k f16 steps) of a mixed row that carries its bias in two spare columns"""
    return ((k + 2 + 31) // 32, (k + 2 + 15) // 16)


def mixed_exponents(fmt, bmax, b2max, tb):
    """(eB, eT) of one segment of mixed rows.  2^eB puts max(|B|, |b2| log2 e) at <= 2^14 (the bias rides in two f16 columns;
    ``b2max`` None: the biases go to the kernel separately), 2^eT the largest value a T column can take (``tb``) times log2 e at
    <= 2^15 -- both inside the f16 range with their low halves out of the subnormals."""
    if b2max is not None:
        bmax = max(bmax, b2max * LOG2E)
    eB = pow2_below(2.0 ** 14, bmax)
    eT = pow2_below(2.0 ** 15, tb * LOG2E)
    if fmt == "mx6":
        # mx6 operands want eT + eB = 0: the accumulators are then base-2 logits themselves (descale = 1) and the fold needs no
        # multiply -- and no running maximum where the loader allows the fixed reference (exp2 + add per logit).  The FP6 planes
        # carry their own block scales, so only the f16 hi planes feel the choice: any exponent that keeps an operand's largest
        # value between 2^-3 and the top of the f16 range leaves its typical values normal (what falls into the subnormals is
        # good to 2^-25 absolute, below the FP6 planes' own step).  Balanced: largest |B| 2^e = largest |T| log2 e 2^-e.
        lo = max(eB - 17, -eT)
        hi = min(eB, 17 - eT, 13)                        # (new eT = -e >= -13: the bias constant 2^(eT - 11) must stay representable)
        if lo <= hi:
            bal = int(round(0.5 * (np.log2(max(tb * LOG2E, 1e-30)) - np.log2(max(bmax, 1e-30)))))
            eB = int(min(max(bal, lo), hi))
            eT = -eB
    return eB, eT


def plane_scale(fmt, hmax):
    """s8 of one segment: the int8 planes' scale, the power of two at or above max|f16(B 2^eB)| / 127 (``hmax``: taken with the
    final eB); 0 selects the FP6 planes, which carry their own block scales (ABI 11)"""
    return 0.0 if fmt == "mx6" else 2.0 ** int(np.ceil(np.log2(max(hmax, 2.0 ** -100) / 127.0)))


def mixed_t_stride(segments):
    """stride of the packed hypothesis rows in floats (jlm_mixed_t_stride): the segments' 128-byte blocks + JLM_MAX_SEGMENTS
    scale floats, rounded up to 16 bytes"""
    nbytes = sum(sg["ldb"] * 4 for sg in segments) + 4 * 8
    return (nbytes + 15) // 16 * 4


def mixed_layout(segments, fmt, split_bias_col, wide_untied=False, shapes=MIXED_SHAPES):
    """Which segments take mixed rows: (their indices, those among them whose biases go to the kernel separately), or None when
    the model stays on split rows.  ``split_bias_col``: the bias column of every segment's split rows (-1: none), empty for a
    model without split rows -- which hosts one form only, ``wide_untied``: the untied H = 512 matrix on int8 planes
    (csrc/jlm_mixed_w.hip: sixteen 32-k blocks per word, one row set)."""
    if not split_bias_col:
        sg = segments[0]
        nv = sg["v_end"] - sg["v_start"]
        ok = wide_untied and fmt == "int8" and len(segments) == 1 and sg["k"] == 512 and nv > 0 and nv * 16 * 128 < (1 << 31)
        return ([0], {0}) if ok else None
    take, xbias = [], set()
    for i, sg in enumerate(segments):
        nv, k = sg["v_end"] - sg["v_start"], sg["k"]
        if nv > 0 and mixed_shape(k) in shapes:
            take.append(i)
        elif nv > 0 and k % 64 == 0 and k <= 256:
            # a contraction that fills its last block (tied k = 256): no columns left for the bias -- rows of k / 32 blocks, the
            # biases (x log2 e) go to the kernel separately (jlm_vocab_lse_mixed, bias2)
            take.append(i)
            xbias.add(i)
        elif not (nv > 0 and k <= 64 and split_bias_col[i] == k):
            return None
    if not take or (xbias and len(xbias) != len(segments)):      # (one bias form per launch)
        return None
    # the packer of the hypothesis rows holds a row's blocks in one wave: 32 blocks per row at most (jlm_mixed_t_stride: -2)
    if sum((segments[i]["k"] // 32) if i in xbias else mixed_shape(segments[i]["k"])[0] for i in take) > 32:
        return None
    # the hybrid launch (mixed + split segments) hosts the mixed bodies with bias columns (k = 200, 100, 50): any other mix stays on split rows
    if len(take) != len(segments) and any(mixed_shape(segments[i]["k"]) not in shapes for i in take):
        return None
    if fmt == "mx6" and len(take) != len(segments):        # (the two-format launch hosts int8 planes only)
        return None
    return take, xbias


# one segment on mixed rows: its index in the model's segment table, the packed words [V_i, ldb], the segment's table entry
# (v_start v_end k t_off ldb) and scales (2^eT, 2^-(eT + eB), s8)
MixedSegment = collections.namedtuple("MixedSegment", "idx packed seg t_scale descale s8")


@dataclasses.dataclass(frozen=True, eq=False)
class MixedRows:
    """The loader's choice for a model whose normaliser runs on mixed rows (a model on split rows has none).  Immutable:
    a candidate form is derived from another (``with_head`` ...) and shares its tensors."""
    fmt: str                     # "mx6" | "int8": the cross-term planes
    segs: tuple                  # MixedSegment, in segment order
    b2_log2: object = None       # biases x log2 e where the rows have no bias columns
    head_split: tuple = ()       # per mixed segment, its first so many words stay on split rows (jlm_vocab_lse_hybrid); () = none
    fixed_ref: bool = False      # the kernel forms without a running maximum may run

    @property
    def idx(self):
        return [s.idx for s in self.segs]

    @property
    def ld_tm(self):
        return mixed_t_stride([s.seg for s in self.segs])

    def with_head(self, cut):
        return dataclasses.replace(self, head_split=(int(cut),) + (0,) * (len(self.segs) - 1))

    def without_first_segment(self):
        return dataclasses.replace(self, segs=self.segs[1:], head_split=())

    def with_fixed_ref(self, flag):
        return dataclasses.replace(self, fixed_ref=bool(flag))
