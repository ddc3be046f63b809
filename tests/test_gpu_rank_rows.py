"""GPU: rank_rows_kernel behind torch.ops.jlm.rank_rows (csrc/jlm_rank.hip, include/jlm_hip.h jlm_rank_rows) on rows the test writes.
The outputs are integer counts, so every output int must EQUAL the definition stated in numpy below: sizes on both sides of the
16-byte load, of a wave's and a workgroup's stride and of the unrolled trip; dyadic logits with ties on both sides of the target; NaN
and +-inf; the flagged rows; level lists of every span size the gather loop distinguishes; rows beyond *n_dev left alone."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
from jlm_amd import ops as _ops                                                           # noqa: E402

pytestmark = pytest.mark.gpu

FILL = -7                                                                                  # what the rank buffer holds before a launch


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _rank_in(row, t, members):
    w = np.asarray(members, dtype=np.int64)
    w = w[(w >= 0) & (w < len(row))]
    with np.errstate(invalid="ignore"):
        v = row[w]
        return int(np.count_nonzero(v > row[t]) + np.count_nonzero((v == row[t]) & (w < t)))


def want_ranks(y, n_cols, target, table, n_levels, n_live):
    """the header's contract in numpy -> (rank [R, n_levels + 1], flags)"""
    R = len(target)
    out = np.full((R, n_levels + 1), FILL, dtype=np.int32)
    flags = 0
    for r in range(min(n_live, R)):
        t = int(target[r])
        out[r] = -1
        if not 0 <= t < n_cols:
            flags |= 2
            continue
        row = y[r, :n_cols]
        if np.isnan(row[t]):
            flags |= 1
            continue
        out[r, 0] = _rank_in(row, t, np.arange(n_cols))
        if table is None:
            continue
        ids, off, lo, hi = table
        for i in range(min(int(off[t + 1] - off[t]), n_levels)):
            e = int(off[t]) + i
            out[r, 1 + i] = _rank_in(row, t, ids[max(int(lo[e]), 0):min(int(hi[e]), len(ids))])
    return out, flags


def run(y, n_cols, target, table=None, n_levels=0, n_dev=None, twice=True):
    """one launch over y [R, ld] f32 (numpy, padding included) -> (rank, flags); launched a second time on the same buffers, the result
    must be the same bits"""
    dev = _dev()
    R, ld = y.shape
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
    yd = torch.from_numpy(np.ascontiguousarray(y)).to(dev)
    tg = up(target)
    tab = [None] * 4 if table is None else [up(a) for a in table]
    nd = None if n_dev is None else up([n_dev])
    rank = torch.full((R, n_levels + 1), FILL, device=dev, dtype=torch.int32)
    flags = torch.zeros(1, device=dev, dtype=torch.int32)
    call = lambda: _ops.backend().rank_rows(yd, ld, n_cols, R, nd, tg, *tab, n_levels, rank, flags)
    call()
    torch.cuda.synchronize()
    got, fl = rank.cpu().numpy(), int(flags.cpu()[0])
    if twice:
        call()
        torch.cuda.synchronize()
        assert np.array_equal(rank.cpu().numpy(), got) and int(flags.cpu()[0]) == fl
    return got, fl


def check(y, n_cols, target, table=None, n_levels=0, n_dev=None):
    got, fl = run(y, n_cols, target, table, n_levels, n_dev)
    want, wfl = want_ranks(y, n_cols, target, table, n_levels, len(target) if n_dev is None else n_dev)
    assert got.tolist() == want.tolist(), (n_cols, np.argwhere(got != want)[:5].tolist())
    assert fl == wfl
    return got


def dyadic_rows(rng, R, n_cols, pad, pad_value):
    """quarters in [-1, 1]: about a ninth of a row equals any target's logit, on both sides of it; +-inf and NaN in a few columns"""
    ld = (n_cols + 3) // 4 * 4 + pad
    y = np.full((R, ld), pad_value, dtype=np.float32)
    y[:, :n_cols] = rng.randint(-4, 5, size=(R, n_cols)) / 4.0
    for r in range(R):
        for v in (np.inf, -np.inf, np.nan):
            y[r, rng.randint(0, n_cols, size=max(1, n_cols // 50))] = v
    return y


def boundary_targets(n_cols):
    """column 0, the last column, both sides of the first and the last 16-byte boundary, and of a workgroup's stride"""
    last4 = 4 * ((n_cols - 1) // 4)
    c = [0, n_cols - 1, 3, 4, last4 - 1, last4, 1023, 1024, n_cols // 2]
    return [x for x in c if 0 <= x < n_cols]


N_COLS = [1, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2003]


@pytest.mark.parametrize("n_cols", N_COLS)
def test_level_a_every_size(n_cols):
    rng = np.random.RandomState(n_cols)
    cand = boundary_targets(n_cols)
    for k, (R, pad, pad_value) in enumerate([(1, 0, np.inf), (3, 0, np.nan), (17, 8, np.inf), (17, 4, -np.inf)]):
        y = dyadic_rows(rng, R, n_cols, pad, pad_value)
        target = np.array([cand[(r + k) % len(cand)] for r in range(R)], dtype=np.int32)
        for r, t in enumerate(target):                      # the target's own logit is a number (NaN targets: below), often +-inf
            if np.isnan(y[r, t]):
                y[r, t] = 0.25
        got = check(y, n_cols, target)
        assert np.all(got >= 0) and np.all(got < n_cols)


def test_tie_rule_and_infinities():
    n = 1025
    y = np.full((6, 1028), 0.5, dtype=np.float32)           # all equal: the rank is the number of lower ids
    target = np.array([0, 1, 511, 512, 1024, 700], dtype=np.int32)
    y[5, :] = -np.inf                                       # ... also among -inf
    y[5, 3] = np.nan
    got = check(y, n, target)
    assert got[:, 0].tolist() == [0, 1, 511, 512, 1024, 699]
    y2 = np.zeros((3, 1028), dtype=np.float32)
    y2[0, 5] = np.inf; y2[0, 9] = np.inf                    # +inf == +inf: the lower id first
    y2[1, 7] = -np.inf
    y2[2, ::2] = np.nan                                     # NaN is never counted
    got = check(y2, n, np.array([9, 7, 1001], dtype=np.int32))
    assert got[:, 0].tolist() == [1, 1024, 500]


def test_flagged_rows_and_rows_left_alone():
    rng = np.random.RandomState(4)
    n = 257
    y = dyadic_rows(rng, 9, n, 4, np.inf)
    y[np.isnan(y)] = 0.0
    target = np.array([5, 100, -1, n, 256, 7, 2 ** 30, -2 ** 31, 3], dtype=np.int32)
    y[1, 100] = np.nan                                      # a NaN target: -1 everywhere, bit 0
    got, fl = run(y, n, target, None, 2)
    want, wfl = want_ranks(y, n, target, None, 2, 9)
    assert got.tolist() == want.tolist() and fl == wfl == 3
    assert got[1].tolist() == got[2].tolist() == got[3].tolist() == got[6].tolist() == got[7].tolist() == [-1, -1, -1]
    assert got[0, 0] >= 0 and got[0, 1:].tolist() == [-1, -1]          # lv_off NULL: level A only
    # only bit 1, only bit 0
    assert run(y[2:4], n, target[2:4])[1] == 2 and run(y[1:2], n, target[1:2])[1] == 1
    # *n_dev below n_rows_max: the later rows' bytes stay as they were (FILL), and a bad target there raises no flag
    for n_dev in (0, 1, 2, 9, 12):
        got = check(y, n, target, None, 1, n_dev=n_dev)
        assert np.all(got[min(n_dev, 9):] == FILL)


def nested_table(rng, n_cols, n_ids, words):
    """ids: a permutation of n_ids of the n_cols words.  words: {word: (sizes, where)} -- the word's level list is nested spans of
    those sizes around its position in ids, the word first / last / anywhere in each; every other word has no entries.
    -> (ids, off, lo, hi)"""
    slot = {"first": lambda k: 100 + 53 * k, "last": lambda k: n_ids - 90 - 53 * k, "any": lambda k: 960 + 7 * k}
    # (the largest span, 1025 entries, fits on the side it needs)
    at = {w: slot[where](k) for k, (w, (_sizes, where)) in enumerate(sorted(words.items()))}
    assert len(set(at.values())) == len(at)
    ids = np.full(n_ids, -1, dtype=np.int32)
    for w, pos in at.items():
        ids[pos] = w
    rest = rng.permutation(np.setdiff1d(np.arange(n_cols), list(words)))
    ids[ids < 0] = rest[:n_ids - len(at)]
    spans = {}
    for w, (sizes, where) in sorted(words.items()):
        pos = at[w]
        lo, hi, out = 0, n_ids, []
        for s in sizes:
            if where == "first":
                a = pos
            elif where == "last":
                a = pos + 1 - s
            else:
                a = rng.randint(max(lo, pos + 1 - s), min(pos, hi - s) + 1)
            assert lo <= a <= pos < a + s <= hi, (w, s, where)
            lo, hi = a, a + s
            out.append((lo, hi))
        spans[w] = out
    assert len(set(ids.tolist())) == n_ids
    off = np.zeros(n_cols + 1, dtype=np.int32)
    for w, sp in spans.items():
        off[w + 1] = len(sp)
    off = np.cumsum(off).astype(np.int32)
    flat = [s for w in sorted(spans) for s in spans[w]]
    lo = np.array([a for a, _b in flat], dtype=np.int32)
    hi = np.array([b for _a, b in flat], dtype=np.int32)
    return ids, off, lo, hi


SIZES = (1025, 257, 256, 256, 255, 1)                      # 256 twice: a level equal to its parent


@pytest.mark.parametrize("n_levels", [0, 1, 6, 32])
def test_levels(n_levels):
    rng = np.random.RandomState(50 + n_levels)
    n_cols, n_ids = 2003, 1990                              # 13 words are in no span: they have no reading
    deep = tuple(range(1025, 1025 - 32 * 31, -31))[:32]     # 32 nested levels
    words = {10: (SIZES, "first"), 20: (SIZES, "last"), 30: (SIZES, "any"), 40: ((1,), "any"), 2002: (deep, "any"), 0: (deep, "first"),
             77: ((n_ids,), "any")}
    table = nested_table(rng, n_cols, n_ids, words)
    assert table[0].tolist() != sorted(table[0].tolist())   # the gather is not the identity
    no_levels = int(np.setdiff1d(np.arange(n_cols), list(words))[5])
    target = np.array([10, 20, 30, 40, 2002, 0, 77, no_levels, 10, 30], dtype=np.int32)
    for R in (1, 3, len(target)):
        y = dyadic_rows(rng, R, n_cols, 4, np.inf)
        for r in range(R):
            if np.isnan(y[r, target[r]]):
                y[r, target[r]] = -0.5
        got = check(y, n_cols, target[:R], table, n_levels)
        if n_levels == 32 and R == len(target):
            assert np.all(got[4] >= 0) and np.all(got[5] >= 0)                  # all 32 levels of the deep words
            assert got[0, 1:7].min() >= 0 and np.all(got[0, 7:] == -1)          # six levels, the rest absent
            assert np.all(got[7, 1:] == -1) and got[7, 0] >= 0                  # a word with no levels
            assert np.all(np.diff(got[4, 1:]) <= 0) and got[0, 3] == got[0, 4]  # nested: ranks cannot grow; equal spans, equal ranks
            assert got[0, 6] == 0 and got[3, 1] == 0                            # a span of the word alone
    # spans that are not nested, reach outside [0, n_ids) or hold an id outside the row are counted as the contract says
    ids, off, lo, hi = [a.copy() for a in table]
    e = int(off[30])
    lo[e:e + 6] = [-5, 900, 0, 1500, 1989, 400]
    hi[e:e + 6] = [300, 1300, n_ids + 50, 1400, 1990, 401]
    ids[100], ids[950] = n_cols, -3
    y = dyadic_rows(rng, 2, n_cols, 0, np.nan)
    y[:, 30] = 0.0
    check(y, n_cols, np.array([30, 30], dtype=np.int32), (ids, off, lo, hi), n_levels)


def test_small_tables():
    """one word, one id; an empty id list with a table; lv_off NULL with columns asked for"""
    y = np.array([[0.25, np.nan, np.nan, np.nan]], dtype=np.float32)
    one = (np.array([0], dtype=np.int32), np.array([0, 2], dtype=np.int32), np.array([0, 0], dtype=np.int32), np.array([1, 1], dtype=np.int32))
    assert check(y, 1, np.array([0], dtype=np.int32), one, 3).tolist() == [[0, 0, 0, -1]]
    y3 = np.array([[0.5, 0.75, 0.5, np.inf]], dtype=np.float32)
    tab = (np.array([2, 1, 0], dtype=np.int32), np.array([0, 0, 0, 2], dtype=np.int32), np.array([0, 1], dtype=np.int32),
           np.array([3, 3], dtype=np.int32))
    assert check(y3, 3, np.array([2], dtype=np.int32), tab, 2).tolist() == [[2, 2, 2]]
    assert check(y3, 3, np.array([1], dtype=np.int32), tab, 2).tolist() == [[0, -1, -1]]
    assert check(y3, 3, np.array([2], dtype=np.int32), None, 2).tolist() == [[2, -1, -1]]


def test_refused_arguments():
    dev = _dev()
    y = torch.zeros((2, 8), device=dev)
    tg = torch.zeros(2, device=dev, dtype=torch.int32)
    rank = torch.full((2, 40), FILL, device=dev, dtype=torch.int32)
    O = _ops.backend()
    for ld, n_cols, n_levels in ((6, 5, 0), (4, 5, 0), (8, 0, 0), (8, 5, -1), (8, 5, 33)):
        with pytest.raises(RuntimeError):
            O.rank_rows(y, ld, n_cols, 2, None, tg, None, None, None, None, n_levels, rank, None)
    with pytest.raises(RuntimeError):                       # a table without its spans
        O.rank_rows(y, 8, 5, 2, None, tg, tg, torch.zeros(6, device=dev, dtype=torch.int32), None, None, 1, rank, None)
    with pytest.raises(RuntimeError):                       # y off the 16-byte grid
        O.rank_rows(y.view(-1)[1:13], 4, 3, 2, None, tg, None, None, None, None, 0, rank, None)
    torch.cuda.synchronize()
    assert bool(torch.all(rank == FILL))


@pytest.mark.parametrize("n_cols", [491520, 491521])
def test_levels_on_both_sides_of_the_bit_plane_limit(n_cols):
    """up to 491 520 words a row's levels read bit planes in LDS (60 KB at that size), above it they gather from the row: the same
    counts from either kernel, at the last size of the one and the first of the other"""
    rng = np.random.RandomState(n_cols % 1000)
    words = {5: (SIZES, "first"), n_cols - 1: (SIZES, "last"), n_cols // 2 + 1: ((1990, 700, 3), "any")}
    table = nested_table(rng, n_cols, 1990, words)
    target = np.array([5, n_cols - 1, n_cols // 2 + 1], dtype=np.int32)
    y = dyadic_rows(rng, 3, n_cols, 0, np.nan)
    y[np.arange(3), target] = 0.25
    got = check(y, n_cols, target, table, 6)
    assert np.all(got[:2] >= 0) and np.all(got[2, :4] >= 0) and np.all(got[2, 4:] == -1)
