"""Exact definitions of the packed operand formats (include/jlm_hip.h: split-f16 rows, int8 "mixed" rows, mx6 rows) and the inputs the
format tests share.  numpy only, and written without a look at tests/fake_hip.py: FakeLib's packers (tests/test_operand_formats_cpu.py)
and the device's (tests/test_gpu_operand_formats.py) are both compared with what stands here, bytes equal.

Every product of two f32 values is formed exactly in float64 (24 x 24 bits fit in 53) and rounded ONCE to the type a definition names;
a value that is rounded twice (first to f32, then to f16) says so.  Differences x - hi are exact in float64 as well."""
import ctypes

import numpy as np

LOG2E = 1.4426950408889634
F16, F32, F64 = np.float16, np.float32, np.float64


def f32_product(a32, b32):
    """f32 of the exact product (one rounding)"""
    return (np.asarray(a32, F32).astype(F64) * F64(F32(b32))).astype(F32)


def f16_once(a32, b32):
    """f16 of the EXACT product (one rounding)"""
    return (np.asarray(a32, F32).astype(F64) * F64(F32(b32))).astype(F16)


def f16_twice(a32, b32):
    """f16 of the f32 product (two roundings)"""
    return f32_product(a32, b32).astype(F16)


def _residual(x32, hi):
    """x - hi, exact (float64)"""
    return x32.astype(F64) - hi.astype(F64)


# ------------------------------------------------------------------------------------------------ split-f16 rows
def split_pair(x32):
    """x (f32, already scaled) -> hi = f16(x), lo = f16(x - hi)"""
    x32 = np.asarray(x32, F32)
    hi = x32.astype(F16)
    with np.errstate(invalid="ignore", over="ignore"):
        lo = _residual(x32, hi).astype(F16)
    return hi, lo


def split_row_bytes(x32):
    """x [rows, k] f32 (scaled), k a multiple of 8 -> the bytes of the split rows: per 8 values [8 x f16 hi][8 x f16 lo]; uint8 [rows, 4 k]"""
    rows, k = x32.shape
    assert k % 8 == 0
    hi, lo = split_pair(x32)
    out = np.empty((rows, k // 8, 2, 8), F16)
    out[:, :, 0, :] = hi.reshape(rows, k // 8, 8)
    out[:, :, 1, :] = lo.reshape(rows, k // 8, 8)
    return out.view(np.uint8).reshape(rows, 4 * k)


def split_planes(bits):
    """bytes of split rows, uint8 [rows, 4 k] -> (hi, lo) f16 [rows, k]"""
    bits = np.ascontiguousarray(bits)
    rows = bits.shape[0]
    k = bits.shape[1] // 4
    v = bits.view(F16).reshape(rows, k // 8, 2, 8)
    return v[:, :, 0, :].reshape(rows, k), v[:, :, 1, :].reshape(rows, k)


def check_split_pairs(bits):
    """what every split row promises, whoever wrote it (bytes of split rows of finite input, uint8 [rows, 4 k]): no NaN / inf;
    |lo| <= ulp(hi) / 2; and lo never moves hi: f16(hi + lo) == hi -- but for the one case a CORRECT lo = f16(x - hi) reaches: a residual
    within 2^-12 of half an ulp of hi rounds UP to exactly that half ulp, hi + lo is then the midpoint between hi and its neighbour on lo's
    side, and for an odd hi round-to-nearest-even names the neighbour (x = 0x1.ac5ffep-3: hi = 0x1.ac4p-3, lo = 2^-14).  Only that exact
    midpoint is let through.
    All of it is ONE comparison: |lo| <= half the distance from hi to its f16 neighbour on lo's side (below that the sum rounds back to hi,
    on it the sum is the midpoint, beyond it hi moves) -- done on the bit fields; up to a million values the sum is also formed and rounded."""
    hi, lo = split_planes(bits)
    hb, lb = hi.view(np.uint16), lo.view(np.uint16)
    assert ((hb & 0x7c00) != 0x7c00).all() and ((lb & 0x7c00) != 0x7c00).all(), "NaN or inf in split rows"
    # |hi| = 1.m 2^(e - 15), e the exponent field (the subnormals share e = 1's spacing): the neighbour away from zero is 2^(max(e, 1) - 25)
    # off, the one towards zero as well unless hi is a power of two above the smallest normal -- there it is half as far
    e = np.maximum((hb >> 10) & 31, 1).astype(np.int32)
    towards_zero = ((hb ^ lb) & 0x8000 != 0) & (lb & 0x7fff != 0) & (hb & 0x7fff != 0)
    e -= (towards_zero & (hb & 0x03ff == 0) & (e > 1)).astype(np.int32)
    ok = np.abs(lo.astype(F32)) <= np.ldexp(F32(1.0), e - 26)
    if hi.size <= 1 << 20:
        h64, l64 = hi.astype(F64), lo.astype(F64)
        with np.errstate(over="ignore"):
            beside = np.nextafter(hi, np.where(np.signbit(lo), F16(-np.inf), F16(np.inf)).astype(F16)).astype(F64)
            beside = np.where(np.isinf(beside), np.copysign(65536.0, beside), beside)         # (the grid point rounding carries 65520 to)
            same = ((h64 + l64).astype(F16) == hi) | (h64 + l64 == (h64 + beside) * 0.5)      # (sums exact in float64)
        assert (same == ok).all(), np.argwhere(same != ok)[:8].tolist()
    assert ok.all(), ("lo moves hi, or |lo| > ulp(hi) / 2, at (row, k):", np.argwhere(~ok)[:8].tolist())


# ------------------------------------------------------------------------------------------------ int8 planes
def int8_planes(hi, lo, s):
    """hi (f16), lo (the residual x - hi, NOT rounded to f16), s a power of two (scalar or one per row, [rows, 1]) ->
    hi8 = rint(hi / s), lo8 = rint(lo / (s / 2048)): ties to even, clipped to +-127"""
    s = np.asarray(s, F64)
    q = lambda v: np.clip(np.rint(v), -127, 127).astype(np.int8)
    return q(np.asarray(hi).astype(F64) / s), q(np.asarray(lo, F64) / (s / 2048.0))


def t_row_scale(amax):
    """the int8 scale of a hypothesis row: the smallest power of two >= amax / 127; 1.0 for an all-zero row"""
    amax = np.asarray(amax, F64)
    m, e = np.frexp(amax / 127.0)                 # = m 2^e, m in [0.5, 1)
    p = np.ldexp(1.0, np.where(m == 0.5, e - 1, e))
    return np.where(amax > 0, p, 1.0).astype(F32)


def t_row_scale_bits(amax32):
    """the same as the kernel spells it: w = f32(amax * f32(1 / 127)), (bits(w) + 0x007fffff) & 0x7f800000"""
    amax32 = np.asarray(amax32, F32)
    w = (amax32 * (F32(1.0) / F32(127.0))).astype(F32)
    b = ((w.view(np.int32) + np.int32(0x007fffff)) & np.int32(0x7f800000)).astype(np.int32)
    return np.where(amax32 > 0, b.view(F32), F32(1.0)).astype(F32)


# ------------------------------------------------------------------------------------------------ mixed rows of a vocabulary block
def mixed_blocks(k, ld_dst):
    """(32-k blocks per row, room for the two bias columns?)"""
    nb = ld_dst // 32
    assert ld_dst % 32 == 0 and nb in ((k + 2 + 31) // 32, (k + 31) // 32)
    return nb, k + 2 <= 32 * nb


def _mixed_hi(src32, k, nb, scale, bias32, bias_scale):
    """-> (x f32 [rows, 32 nb] zero behind k, the f16 plane with the bias columns, mask of the real columns)"""
    rows = src32.shape[0]
    x = np.zeros((rows, 32 * nb), F32)
    x[:, :k] = f32_product(src32[:, :k], scale)
    hi = x.astype(F16)
    if k + 2 <= 32 * nb:
        xb = f32_product(bias32, bias_scale) if bias32 is not None else np.zeros(rows, F32)
        bh = xb.astype(F16)
        hi[:, k] = bh
        hi[:, k + 1] = (_residual(xb, bh) * 2048.0).astype(F16)
    return x, hi, (np.arange(32 * nb) < k)[None, :]


def mixed_row_bytes(src32, k, ld_dst, scale, bias32, bias_scale, s8):
    """int8 form of jlm_pack_mixed: src [rows, >= k] f32, bias [rows] f32 or None -> uint8 [rows, 128 nb], per 32 k-values
    [32 x f16 hi | 32 x int8 hi8 | 32 x int8 lo8].  x = f32(src scale), hi = f16(x), planes of hi and x - hi with scale s8; the
    bias columns (when there is room): k = f16(xb), k + 1 = f16((xb - f16(xb)) 2048), xb = f32(bias bias_scale); zero planes behind k"""
    nb, _ = mixed_blocks(k, ld_dst)
    rows = src32.shape[0]
    x, hi, real = _mixed_hi(src32, k, nb, scale, bias32, bias_scale)
    h8, l8 = int8_planes(x.astype(F16), _residual(x, x.astype(F16)), s8)
    h8, l8 = np.where(real, h8, 0).astype(np.int8), np.where(real, l8, 0).astype(np.int8)
    out = np.empty((rows, nb, 128), np.uint8)
    out[:, :, :64] = hi.reshape(rows, nb, 32).view(np.uint8).reshape(rows, nb, 64)
    out[:, :, 64:96] = h8.reshape(rows, nb, 32).view(np.uint8)
    out[:, :, 96:128] = l8.reshape(rows, nb, 32).view(np.uint8)
    return out.reshape(rows, nb * 128)


# ------------------------------------------------------------------------------------------------ FP6 (e2m3) planes of the mx6 rows
def _e2m3_codes(v, byte):
    """6-bit codes (sign, 2 exponent bits, 3 mantissa bits) of v / 2^(byte - 127): nearest grid point (steps 0.125 below 2, 0.25 below 4,
    0.5 up to 7.5), ties to even, saturating at 7.5; the sign bit is v's own, of a zero as well"""
    a = np.minimum(np.abs(np.ldexp(v.astype(F64), (127 - byte).astype(np.int64))), 7.5)
    mul = np.where(a < 2.0, 8.0, np.where(a < 4.0, 4.0, 2.0))
    off = np.where(a < 2.0, 0, np.where(a < 4.0, 8, 16))
    return (np.rint(a * mul).astype(np.int64) + off) | (np.signbit(v).astype(np.int64) << 5)


def _block_byte(amax):
    """E8M0 byte of a block: the smallest power of two s = 2^(byte - 127) with amax <= 7.5 s; 0 for an all-zero block"""
    m, e = np.frexp(amax.astype(F64))             # amax = m 2^e, m in [0.5, 1): 7.5 s >= amax  <=>  0.9375 2^(log2 s + 3) >= m 2^e
    ex = np.where(m <= 0.9375, e - 3, e - 2)
    return np.where(amax > 0, np.clip(ex + 127, 0, 254), 0).astype(np.int64)


def fp6_plane(v):
    """v [rows, nb, 32] -> (24 bytes per block: the 32 codes, 6 bits each, little-endian; the block's scale byte)"""
    byte = _block_byte(np.abs(v).max(axis=2))
    code = _e2m3_codes(v, byte[:, :, None])
    bits = ((code[..., None] >> np.arange(6)) & 1).astype(np.uint8).reshape(v.shape[0], v.shape[1], 192)
    return np.packbits(bits, axis=2, bitorder="little"), byte.astype(np.uint8)


def _mx6_planes(x, k, nb):
    rows = x.shape[0]
    real = (np.arange(32 * nb) < k)[None, :]
    h = x.astype(F16)
    ph, bh = fp6_plane(np.where(real, h.astype(F64), 0.0).reshape(rows, nb, 32))
    pl, bl = fp6_plane(np.where(real, _residual(x, h), 0.0).reshape(rows, nb, 32))
    return ph, bh, pl, bl


def mx6_row_bytes(src32, k, ld_dst, scale, bias32, bias_scale):
    """mx6 form of jlm_pack_mixed (s8 = 0): the f16 plane of mixed_row_bytes; granules 4-6 the FP6 planes of the real k-values --
    half 0 = hi6 (of the f16 hi), half 1 = lo6 (of x - hi): [half 0 bytes 0-15 | half 0 16-23, half 1 16-23 | half 1 0-15] --;
    granule 7: zero, but in a row's block 0 bytes j / 8 + j = the scale bytes of block j's hi6 / lo6 plane"""
    nb, _ = mixed_blocks(k, ld_dst)
    assert nb <= 8
    rows = src32.shape[0]
    x, hi, _ = _mixed_hi(src32, k, nb, scale, bias32, bias_scale)
    ph, bh, pl, bl = _mx6_planes(x, k, nb)
    out = np.zeros((rows, nb, 128), np.uint8)
    out[:, :, :64] = hi.reshape(rows, nb, 32).view(np.uint8).reshape(rows, nb, 64)
    out[:, :, 64:80], out[:, :, 80:88], out[:, :, 88:96], out[:, :, 96:112] = ph[:, :, :16], ph[:, :, 16:], pl[:, :, 16:], pl[:, :, :16]
    out[:, 0, 112:112 + nb], out[:, 0, 120:120 + nb] = bh, bl
    return out.reshape(rows, nb * 128)


# ------------------------------------------------------------------------------------------------ packed hypothesis rows
def t_stride(segs):
    """row stride (4-byte units) of packed hypothesis rows; segs = [(k, t_off, nb)]: the blocks + 8 floats of row scales"""
    return (sum(128 * nb for _, _, nb in segs) + 32 + 15) // 16 * 4


def t_row_bytes(T32, segs, t_scales, mx6):
    """T [n, ldt] f32 (the rows to pack, in packed order), segs = [(k, t_off, nb)], t_scales[i] = 2^eT_i ->
    (bytes uint8 [n, 4 ld_tm] ROW-major: every segment's blocks, then 8 floats; written: bool mask of the bytes the packer defines).
    The multiplier of segment i is m = f32(2^eT_i log2 e).

    int8 form (jlm_pack_t_mixed): hi = f16 of the EXACT product T m (one rounding); the row's scale per segment s = t_row_scale(max |hi|)
    over the real k-values, at float i of the row's last 8; hi8 / lo8 = int8_planes(hi, f32(T m) - hi, s), zero behind k.
    mx6 form (jlm_pack_t_mixed6): hi = f16(f32(T m)) (two roundings); the FP6 planes with the halves SWAPPED against the vocabulary rows --
    half 0 = lo6, half 1 = hi6 --; of granule 7 only bytes j / 8 + j (j < nb) of a segment's block 0 are written (lo6 / hi6 scale bytes),
    and none of the 8 floats.
    Both: the bias constants 2^eT and 2^(eT - 11) at f16 columns k, k + 1 where 32 nb >= k + 2, zero behind them."""
    n = T32.shape[0]
    ld_tm = t_stride(segs)
    out = np.zeros((n, 4 * ld_tm), np.uint8)
    written = np.zeros((n, 4 * ld_tm), bool)
    scales = out[:, 4 * ld_tm - 32:].view(F32)
    off = 0
    for i, (k, t_off, nb) in enumerate(segs):
        m = F32(F32(t_scales[i]) * F32(LOG2E))
        tv = T32[:, t_off:t_off + k]
        x = np.zeros((n, 32 * nb), F32)
        x[:, :k] = f32_product(tv, m)
        hi = np.zeros((n, 32 * nb), F16)
        hi[:, :k] = f16_twice(tv, m) if mx6 else f16_once(tv, m)
        blk = out[:, off:off + 128 * nb].reshape(n, nb, 128)
        wr = written[:, off:off + 128 * nb].reshape(n, nb, 128)
        if mx6:
            ph, bh, pl, bl = _mx6_planes(x, k, nb)
            blk[:, :, 64:80], blk[:, :, 80:88], blk[:, :, 88:96], blk[:, :, 96:112] = pl[:, :, :16], pl[:, :, 16:], ph[:, :, 16:], ph[:, :, :16]
            blk[:, 0, 112:112 + nb], blk[:, 0, 120:120 + nb] = bl, bh
            wr[:, :, :112] = True
            wr[:, 0, 112:112 + nb] = True
            wr[:, 0, 120:120 + nb] = True
        else:
            s = t_row_scale(np.abs(hi[:, :k].astype(F64)).max(axis=1))
            h8, l8 = int8_planes(hi, _residual(x, hi), s[:, None].astype(F64))
            real = (np.arange(32 * nb) < k)[None, :]
            blk[:, :, 64:96] = np.where(real, h8, 0).astype(np.int8).reshape(n, nb, 32).view(np.uint8)
            blk[:, :, 96:128] = np.where(real, l8, 0).astype(np.int8).reshape(n, nb, 32).view(np.uint8)
            scales[:, i] = s
            wr[:] = True
            written[:, 4 * ld_tm - 32 + 4 * i:4 * ld_tm - 32 + 4 * i + 4] = True
        if k + 2 <= 32 * nb:
            hi[:, k] = F16(t_scales[i])
            hi[:, k + 1] = F16(float(t_scales[i]) / 2048.0)
        blk[:, :, :64] = hi.reshape(n, nb, 32).view(np.uint8).reshape(n, nb, 64)
        off += 128 * nb
    return out, written


def tm_image_index(n_rows, ld_tm):
    """The device keeps packed hypothesis rows GRANULE-major in blocks of 32 rows (csrc/jlm_mixed_body.h): of row r the 16-byte granule g
    lies at byte (r / 32) 128 ld_tm + 512 g + 16 (r % 32), its 8 scale floats at (r / 32) 128 ld_tm + 32 (4 ld_tm - 32) + 32 (r % 32).
    -> int64 [ceil(n_rows / 32) 32, 4 ld_tm]: byte b of ROW-major row r (granules, then the 8 floats) is byte index[r, b] of the image.
    A bijection: image[index] is the row-major form of the whole buffer and image2[index] = rows the way back."""
    r32 = (n_rows + 31) // 32 * 32
    rb = 4 * ld_tm
    r = np.arange(r32)[:, None]
    b = np.arange(rb)[None, :]
    gran = (r // 32) * 32 * rb + (b // 16) * 512 + (r % 32) * 16 + b % 16
    scal = (r // 32) * 32 * rb + 32 * (rb - 32) + (r % 32) * 32 + (b - (rb - 32))
    idx = np.where(b < rb - 32, gran, scal).astype(np.int64)
    assert len(np.unique(idx)) == r32 * rb
    return idx


# ------------------------------------------------------------------------------------------------ inputs
def tie_values(scale32):
    """f32 inputs t whose f32 product with scale32 lands on (or next to) an f16 rounding tie while the exact product does not: the
    midpoints of the f16 values in [1024, 2048) divided by the scale, each quotient with its two f32 neighbours (3 072 values).  Those
    that round differently once and twice come first; there are at least 100 (514 for f32(2^10 log2 e))"""
    scale32 = F32(scale32)
    mid = np.arange(1024, 2048, dtype=F64) + 0.5
    q = (mid / F64(scale32)).astype(F32)
    t = np.stack([np.nextafter(q, F32(0.0)), q, np.nextafter(q, F32(np.inf))], axis=1).reshape(-1).astype(F32)
    differ = f16_once(t, scale32) != f16_twice(t, scale32)
    assert differ.sum() >= 100, differ.sum()
    return np.concatenate([t[differ], t[~differ]])


def tie_rows(scale32, rows, k):
    """[rows, k] f32 of tie_values(scale32), the values that round differently first, with alternating signs"""
    t = tie_values(scale32)
    x = np.resize(t, rows * k).reshape(rows, k).copy()
    x[:, 1::2] *= F32(-1.0)
    return x


def split_values(rng, rows, k, scale):
    """[rows, k] f32 inputs for a split-row packer at a power-of-two `scale`: N(0, 1) with, scattered over every row, +-0, products that
    are f16-subnormal, a residual that is f16-subnormal, exactly +-65504 / scale, and f16 rounding ties (midpoints between neighbouring f16
    values, which the scale maps to exactly) -- no f32-subnormal input"""
    inv = F64(1.0) / F64(scale)
    x = np.clip(rng.standard_normal((rows, k)), -3.9, 3.9)          # (3.9 x 2^14 < 65504)
    special = np.concatenate([
        [0.0, -0.0, 65504.0, -65504.0],
        np.ldexp(rng.uniform(1.0, 2.0, 6), rng.integers(-24, -14, 6)) * rng.choice([-1.0, 1.0], 6),      # hi f16-subnormal
        [2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -14 - 2.0 ** -25],                               # ... and ties among the subnormals
        (1.0 + rng.integers(0, 1024, 6) / 1024.0) * (1.0 + rng.uniform(0.1, 0.9, 6) * 2.0 ** -21),         # lo in [2^-24, 2^-14)
        (np.arange(1024, 2048, 171) + 0.5) * rng.choice([-1.0, 1.0], 6),                                 # ties: hi odd / even
        (np.arange(1025, 2048, 171) + 0.5) / 1024.0,
        [2047.5, 1023.75],                                                               # ties that carry into the next binade
    ]) * inv
    special = special.astype(F32)
    assert (np.abs(special[special != 0]) >= 2.0 ** -126).all(), "f32-subnormal input"
    flat = x.reshape(-1)
    pos = rng.permutation(flat.size)[:min(flat.size, max(len(special), flat.size // 3))]
    flat[pos] = np.resize(special, len(pos))
    return flat.reshape(rows, k).astype(F32)


# ------------------------------------------------------------------------------------------------ the cases, shared by the CPU and GPU tests
# A case packs into a destination pre-filled with SENT bytes through library `L` (the device's, or FakeLib) and compares EVERY byte of the
# destination: the written region with the definition above, everything else with the sentinel.  `mem` moves buffers: put(array) -> handle,
# ptr(handle, byte_offset), get(handle) -> its bytes (uint8, flat), stream.
SENT = 0xA5            # 0xa5a5 is a finite f16, 0xa5a5a5a5 a finite f32, 0xa5 not an int8 the cases produce by accident


class HostMem:
    """buffers of the numpy restatement: plain arrays; FakeLib keeps packed hypothesis rows ROW-major (the device: tm_image_index)"""
    stream = 0
    granule_major = False

    @staticmethod
    def put(a):
        return np.array(a, copy=True, order="C")

    @staticmethod
    def ptr(h, off=0):
        return h.ctypes.data + off

    @staticmethod
    def get(h):
        return h.reshape(-1).view(np.uint8).copy()


def sentinel(*shape):
    return np.full(shape, SENT, np.uint8)


def assert_bytes(got, want, what):
    got, want = np.asarray(got).reshape(want.shape), np.asarray(want)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (what, "%d bytes differ; first (index..., got, want):" % len(bad),
                           [tuple(b.tolist()) + (int(got[tuple(b)]), int(want[tuple(b)])) for b in bad[:8]])


def pad16(k):
    return (k + 15) // 16 * 16


def case_pack_split(L, mem, rows, k, src, col0, scale, ld_dst):
    """jlm_pack_split_f16 of columns [col0, col0 + k) of src [rows, ld] at `scale` into rows of stride ld_dst: x = f32(src scale), the blocks
    covering pad16(k) written (zero behind k), the rest of a destination row untouched.  -> the destination's bytes [rows, 4 ld_dst]"""
    ld = src.shape[1]
    hs, hd = mem.put(src), mem.put(sentinel(rows, 4 * ld_dst))
    assert L.jlm_pack_split_f16(mem.ptr(hs, 4 * col0), rows, k, ld, float(scale), mem.ptr(hd), ld_dst, mem.stream) == 0
    x = np.zeros((rows, pad16(k)), F32)
    x[:, :k] = f32_product(src[:, col0:col0 + k], scale)
    want = sentinel(rows, 4 * ld_dst)
    want[:, :4 * pad16(k)] = split_row_bytes(x)
    got = mem.get(hd).reshape(rows, 4 * ld_dst)
    assert_bytes(got, want, "jlm_pack_split_f16 rows=%d k=%d ld=%d ld_dst=%d scale=%r" % (rows, k, ld, ld_dst, float(scale)))
    check_split_pairs(got[:, :4 * pad16(k)])
    return got


def case_pack_split_col(L, mem, rows, v, scale, ld_dst, col):
    """jlm_pack_split_f16_col: hi / lo of f32(v scale) at column col; the 15 other values of the touched blocks and every other block stay"""
    hv, hd = mem.put(v), mem.put(sentinel(rows, 4 * ld_dst))
    assert L.jlm_pack_split_f16_col(mem.ptr(hv), rows, float(scale), mem.ptr(hd), ld_dst, col, mem.stream) == 0
    hi, lo = split_pair(f32_product(v, scale))
    want = sentinel(rows, 4 * ld_dst).view(F16).reshape(rows, ld_dst // 8, 2, 8)
    want[:, col // 8, 0, col % 8] = hi
    want[:, col // 8, 1, col % 8] = lo
    assert_bytes(mem.get(hd).reshape(rows, 4 * ld_dst), want.view(np.uint8).reshape(rows, 4 * ld_dst),
                 "jlm_pack_split_f16_col rows=%d ld_dst=%d col=%d" % (rows, ld_dst, col))


def odd_codebook(n_codes):
    """f32 bit patterns a copy must not touch: -0.0, a subnormal, inf, a NaN with a payload, then ordinary values"""
    bits = np.array([0x80000000, 0x00000123, 0x7f800000, 0x7fc12345, 0xff800001, 0x3f800000], np.uint32)
    book = (np.arange(n_codes, dtype=np.float32) * F32(0.37) - F32(11.0)).view(np.uint32)
    book[:min(n_codes, len(bits))] = bits[:n_codes]
    return book


def case_dequant_u8(L, mem, rows, k, n_codes, code):
    """jlm_dequant_u8: dst[r][c] = codebook[code[r][c]] bit for bit, +0.0 for a code >= n_codes; code [rows, ld_code] uint8 with ld_code > k, the
    destination's stride ld_dst > k; columns behind k untouched"""
    ld_code, ld_dst = code.shape[1], k + 3
    book = odd_codebook(n_codes)
    hc, hb, hd = mem.put(code), mem.put(book.view(F32)), mem.put(sentinel(rows, 4 * ld_dst))
    assert L.jlm_dequant_u8(mem.ptr(hc), rows, k, ld_code, mem.ptr(hb), n_codes, mem.ptr(hd), ld_dst, mem.stream) == 0
    table = np.zeros(256, np.uint32)
    table[:n_codes] = book
    want = sentinel(rows, 4 * ld_dst).view(np.uint32)
    want[:, :k] = table[code[:, :k]]
    assert_bytes(mem.get(hd).reshape(rows, 4 * ld_dst), want.view(np.uint8), "jlm_dequant_u8 rows=%d k=%d n_codes=%d" % (rows, k, n_codes))


def mixed_case_inputs(rng, rows, k, eB, s8):
    """src [rows, k + 4] (a stride wider than k), bias [rows] for a vocabulary block packed at scale 2^eB with int8 scale s8 (a power of two):
    N(0, 0.08) with quotients hi / s8 and lo / (s8 / 2048) ON .5 (ties to even, both parities and signs), values whose planes clip at +-127
    (|hi| up to 2^14 against s8), +-0, and biases with zeros among them"""
    sc = 2.0 ** eB
    src = (rng.standard_normal((rows, k + 4)) * 0.08)
    n = np.arange(-6, 7)
    hi_ties = (n + 0.5) * s8                                   # hi / s8 = n + .5; f16-exact (s8 a power of two, few bits)
    lo_ties = 2048.0 * s8 + (n + 0.5) * s8 / 2048.0            # hi = 2048 s8 (24 bits in all: exact in f32), lo / (s8 / 2048) = n + .5
    clip = np.array([130.0, -127.5, 126.5, 127.5, -4000.0]) * s8
    lo_clip = 32768.0 * s8 * (1 + 2.0 ** -11 * 0.9)            # a residual of 0.9 half-ulps of a large hi: far beyond 127 steps
    special = np.concatenate([hi_ties, lo_ties, clip, [lo_clip, -lo_clip, 0.0, -0.0]]) / sc
    flat = src.reshape(-1)
    pos = rng.permutation(flat.size)[:max(len(special), flat.size // 4)]
    flat[pos] = np.resize(special, len(pos))
    bias = (rng.standard_normal(rows) * 0.3)
    bias[::5] = 0.0
    return src.astype(F32), bias.astype(F32)


def case_pack_mixed(L, mem, rows, k, src, bias, eB, s8, spare):
    """jlm_pack_mixed of src [rows, ld] (ld > k): `spare` -- ld_dst = 32 ceil((k + 2) / 32), the bias rides in columns k, k + 1 -- or not
    (ld_dst = k, k a multiple of 32: `bias` is ignored); s8 > 0: int8 planes, s8 = 0: mx6 rows.  Every byte of the rows is defined."""
    ld_dst = (k + 2 + 31) // 32 * 32 if spare else k
    sc, bsc = 2.0 ** eB, 2.0 ** eB * LOG2E
    hs, hd = mem.put(src), mem.put(sentinel(rows + 1, 4 * ld_dst))
    hb = mem.put(bias) if bias is not None else None
    assert L.jlm_pack_mixed(mem.ptr(hs), rows, k, src.shape[1], mem.ptr(hb) if bias is not None else None, sc, bsc, float(s8),
                            mem.ptr(hd), ld_dst, mem.stream) == 0
    want = sentinel(rows + 1, 4 * ld_dst)           # (one more row than is packed: it stays)
    want[:rows] = mixed_row_bytes(src, k, ld_dst, sc, bias, bsc, s8) if s8 else mx6_row_bytes(src, k, ld_dst, sc, bias, bsc)
    got = mem.get(hd).reshape(rows + 1, 4 * ld_dst)
    assert_bytes(got, want, "jlm_pack_mixed rows=%d k=%d ld_dst=%d s8=%r bias=%s" % (rows, k, ld_dst, s8, bias is not None))
    return got


def t_case_segments(widths):
    """[(k, t_off, nb)] of consecutive segments: a contraction that fills its last block has no bias columns"""
    segs, off = [], 0
    for k in widths:
        segs.append((k, off, k // 32 if k % 32 == 0 else (k + 2 + 31) // 32))
        off += k
    return segs, off


def t_case_rows(rng, n, segs, ldt, eT):
    """T [n, ldt] f32 for the hypothesis-row packers at t_scale = 2^eT, a different kind of row in turn: (0) tie_values of the multiplier
    f32(2^eT log2 e), the ones that round differently once and twice first; (1) all zero: scale 1.0; (2) per segment the largest |hi| exactly
    127 x 8: scale 8; (3) the next f16 above it: scale 16; (4) an ordinary row x 2^-30; (5) every other value zero; (6) an ordinary row"""
    m = F32(F32(2.0 ** eT) * F32(LOG2E))
    T = (np.tanh(rng.standard_normal((n, ldt))) * rng.uniform(1e-3, 0.2, size=(n, 1))).astype(F32)
    ties = tie_values(m)
    for r in range(n):
        kind = r % 7
        if kind == 0:
            T[r] = np.resize(np.roll(ties, -r), ldt) * np.where(np.arange(ldt) % 3 == 2, -1, 1)
        elif kind == 1:
            T[r] = 0.0
        elif kind in (2, 3):
            for k, t_off, _ in segs:
                T[r, t_off + (r % k)] = -F32((1016.0 if kind == 2 else 1016.5) / F64(m))
        elif kind == 4:
            T[r] *= F32(2.0 ** -30)
        elif kind == 5:
            T[r, ::2] = 0.0
    return T


def case_pack_t(L, mem, widths, R, with_rows, with_n_dev, mx6, eT=10, seed=0):
    """jlm_pack_t_mixed / jlm_pack_t_mixed6 of R listed rows (n_dev = R - 2 of them when with_n_dev) into the granule-major image of
    ceil(R / 32) x 32 rows: every byte the definition (t_row_bytes) marks as written, in place; every other byte of the image -- the rows from
    n_dev on, the rest of the 32-row block, the scale floats of segments the launch has not, the unused bytes of an mx6 row -- the sentinel.
    -> (T rows in packed order, the image's bytes ROW-major [rows32, 4 ld_tm], the definition's bytes, its mask)"""
    from jlm_amd import _lib
    rng = np.random.default_rng(1000 * sum(widths) + 10 * R + seed)
    segs, ldt = t_case_segments(widths)
    n_seg = len(segs)
    ld_tm = t_stride(segs)
    G = R + 5
    T = t_case_rows(rng, G, segs, ldt, eT)
    rows = np.array([0] + [G - i for i in range(1, R)], np.int32) if with_rows else None       # (row 0, then from the end backwards)
    n = max(min(R - 2, R), 0) if with_n_dev else R
    cs = (_lib.Segment * n_seg)(*[_lib.Segment(0, 1, k, t_off, None, 32 * nb) for k, t_off, nb in segs])
    ts = (ctypes.c_float * n_seg)(*[2.0 ** eT] * n_seg)
    assert L.jlm_mixed_t_stride(cs, n_seg) == ld_tm
    r32 = (R + 31) // 32 * 32
    hT, hTm = mem.put(T), mem.put(sentinel(r32 * 4 * ld_tm))
    hr = mem.put(rows) if with_rows else None
    hn = mem.put(np.array([R - 2], np.int32)) if with_n_dev else None
    fn = L.jlm_pack_t_mixed6 if mx6 else L.jlm_pack_t_mixed
    assert fn(cs, ts, n_seg, mem.ptr(hT), ldt, mem.ptr(hr) if with_rows else None, R, mem.ptr(hn) if with_n_dev else None,
              mem.ptr(hTm), ld_tm, mem.stream) == 0
    Tp = T[rows[:n]] if with_rows else T[:n]
    body, written = t_row_bytes(Tp, segs, [2.0 ** eT] * n_seg, mx6)
    want = sentinel(r32, 4 * ld_tm)
    want[:n][written] = body[written]
    return Tp, mem.get(hTm), want, (body, written, segs, ld_tm, r32)


# ---- the drivers: what one parametrised test runs, the same on the host and on the device
SPLIT_ROWS, SPLIT_K, SPLIT_SCALES = (1, 5, 257), (1, 7, 8, 9, 15, 16, 17, 200, 512), (2.0 ** -3, 2.0 ** 10, 2.0 ** 14)
COL_ROWS = (1, 256, 257)
DEQUANT_CODES, DEQUANT_K = (1, 2, 255, 256), (1, 3, 4, 5, 257)
# (k = 30, 31 -- bias columns that would exactly fill / spill out of a block -- are no multiples of 4: the launcher refuses them, -1, and the
#  case is that it does and writes nothing; 28 and 32 are their nearest neighbours it takes)
MIXED_K, MIXED_ROWS = (28, 30, 31, 32, 36, 52, 100, 200, 256), (1, 9, 300)
T_WIDTHS, T_ROWS = ([200, 100, 52], [256], [36, 128]), (1, 3, 4, 5, 31, 32, 33, 75)


def run_pack_split(L, mem, rows, k):
    """both source strides (ld = k; ld = k + 12 as a column-offset view), both destination strides, the three power-of-two scales"""
    rng = np.random.default_rng(100 * rows + k)
    for scale in SPLIT_SCALES:
        for ld, col0 in ((k, 0), (k + 12, 5)):
            src = split_values(rng, rows, ld, scale)
            for ld_dst in (pad16(k), pad16(k) + 32):
                case_pack_split(L, mem, rows, k, src, col0, scale, ld_dst)


def run_pack_split_ties(L, mem):
    """the scale that is no power of two, f32(2^10 log2 e), on tie_values: x = f32(src scale) -- ONE f32 rounding -- then split_pair(x).  If
    the packer rounded hi from the exact product and took lo from the f32 one (or the other way round), hi and lo would disagree on
    hundreds of these values"""
    m = F32(F32(1024.0) * F32(LOG2E))
    src = tie_rows(m, 5, 200)
    got = case_pack_split(L, mem, 5, 200, src, 0, m, 208)
    hi, _ = split_planes(got[:, :4 * 208])
    assert (hi[:, :200] != f16_once(src, m)).sum() >= 100           # the case bites: the once-rounded hi is another


def run_pack_split_col(L, mem, rows):
    rng = np.random.default_rng(rows)
    for ld_dst in (16, 48):
        for col in sorted({0, 7, 8, 15, ld_dst - 1}):
            v = split_values(rng, rows, 1, 2.0 ** 10).reshape(-1)
            case_pack_split_col(L, mem, rows, v, 2.0 ** 10, ld_dst, col)
    m = F32(F32(1024.0) * F32(LOG2E))
    case_pack_split_col(L, mem, rows, tie_rows(m, rows, 1).reshape(-1), m, 16, 9)


def run_dequant_u8(L, mem, n_codes, k):
    """rows x ceil(k / 4) threads cross a 256-thread boundary; every code 0 .. 255 occurs where there is room, those >= n_codes give +0.0"""
    rng = np.random.default_rng(1000 * n_codes + k)
    rows = {1: 300, 3: 257, 4: 257, 5: 129, 257: 5}[k]
    code = rng.integers(0, 256, size=(rows, k + 5), dtype=np.uint8)
    code.reshape(-1)[:256] = np.arange(256, dtype=np.uint8)[:min(256, code.size)]
    case_dequant_u8(L, mem, rows, k, n_codes, code)


def run_pack_mixed(L, mem, rows, k, mx6):
    """bias given and NULL, the proper int8 scale and one a power of two too small; where k fills its last block also ld_dst = k (no bias columns)"""
    rng = np.random.default_rng(7 * rows + k + (1 if mx6 else 0))
    if k % 4:                            # refused by the launcher (and by the restatement): nothing may be written
        src, bias = mixed_case_inputs(rng, rows, k, 8, 1.0)
        ld_dst = (k + 2 + 31) // 32 * 32
        hs, hb, hd = mem.put(src), mem.put(bias), mem.put(sentinel(rows, 4 * ld_dst))
        assert L.jlm_pack_mixed(mem.ptr(hs), rows, k, k + 4, mem.ptr(hb), 256.0, 256.0 * LOG2E, 0.0 if mx6 else 1.0, mem.ptr(hd), ld_dst, mem.stream) == -1
        assert_bytes(mem.get(hd), sentinel(rows * 4 * ld_dst), "a refused jlm_pack_mixed wrote")
        return
    eB = 4 if mx6 else 8
    for s8 in ((0.0,) if mx6 else (1.0, 0.5)):
        src, bias = mixed_case_inputs(rng, rows, k, eB, s8 or 1.0)
        for spare in ((True, False) if k % 32 == 0 else (True,)):
            if (k + 2 + 31) // 32 > 8 and spare:
                continue                 # a row holds at most eight blocks (include/jlm_hip.h): k = 256 only without bias columns
            for b in (bias, None):
                case_pack_mixed(L, mem, rows, k, src, b, eB, s8, spare)


def run_pack_t(L, mem, widths, R):
    """the int8 and the mx6 packer on the same rows, with and without a `rows` map, with n_dev = R - 2 and with every row"""
    for with_rows in (False, True):
        for with_n_dev in (True, False):
            planes = {}
            for mx6 in (False, True):
                Tp, got, want, (body, written, segs, ld_tm, r32) = case_pack_t(L, mem, widths, R, with_rows, with_n_dev, mx6)
                idx = tm_image_index(R, ld_tm)
                assert_bytes(got[idx] if mem.granule_major else got.reshape(want.shape), want, "%s widths=%r R=%d rows=%s n_dev=%s (row, byte of the row-major row)"
                             % ("jlm_pack_t_mixed6" if mx6 else "jlm_pack_t_mixed", widths, R, with_rows, with_n_dev))
                planes[mx6] = (Tp, body)
            # the int8 form shows the once-rounded f16 plane, the mx6 form the twice-rounded one: on the tie rows they differ
            (Tp, b8), (_, b6) = planes[False], planes[True]
            if len(Tp):                  # (row 0 is a tie row in either order)
                off, differ = 0, 0
                for k, t_off, nb in segs:
                    h8 = b8[:, off:off + 128 * nb].reshape(len(Tp), nb, 128)[:, :, :64]
                    h6 = b6[:, off:off + 128 * nb].reshape(len(Tp), nb, 128)[:, :, :64]
                    differ += int((h8.view(F16) != h6.view(F16)).sum())
                    off += 128 * nb
                assert differ >= 100, differ
