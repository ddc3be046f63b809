"""GPU: the ring kernel of the T projection (gemm_split3_kernel: four stages, the fragments of the next k-step read while the MFMAs of this
one run; DESIGN.md 4.1 "chain trips") against the two-stage tile kernel gemm_split_kernel<Cfg64>, which feeds every accumulator the same
MFMAs in the same order -- so the comparison is ==, bit for bit, on the whole output buffer.

The oracle is reached by SHAPE, not by environment: jlm_gemm_nt_split takes the ring kernel while the launch has at most 256 tiles of
64 x 64, so the same problem is launched again with the static row bound raised until it has more (2 752 rows at N = 352: 43 x 6 = 258
tiles) and the extra rows mapped to -1 in both the gather and the scatter map: zero rows that store nothing.  Both answers of
jlm_gemm_nt_split_form are asserted.

Cases: M = 1, 63, 64, 65, 200 (below, at and above a tile; four row tiles); N = 40, 256, 352 (a partial column tile, full ones, the
decode's); K = 16, 32, 64, 96, 512 (half a k-step, fewer k-steps than ring stages, three, sixteen); gathered operand rows with a -1
entry; output rows scattered by c_map; device-side counts 0, 1 and M; every output element no launch may touch keeps a sentinel."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
from jlm_amd import _lib                                                                               # noqa: E402

gpu = pytest.mark.gpu
JLM_T_SPLIT3_LINEAR, JLM_T_SPLIT3_XCD, JLM_T_CFG64 = 0, 1, 2       # include/jlm_hip.h
SENTINEL = -77.25
MS = [1, 63, 64, 65, 200]


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return _lib.lib()


def _st():
    return torch.cuda.current_stream().cuda_stream


def oracle_bound(N):
    """smallest static row bound (a multiple of 64) at which M x N has more than 256 tiles of 64 x 64"""
    return (256 // ((N + 63) // 64) + 1) * 64


def split_rows(L, x, scale):
    """[rows, K] f32 on the device -> split rows of the same stride"""
    rows, K = x.shape
    out = torch.zeros_like(x)
    assert L.jlm_pack_split_f16(x.data_ptr(), rows, K, K, float(scale), out.data_ptr(), K, _st()) == 0
    return out


class Problem:
    """operands of one (N, K): 210 storage rows of A, N rows of B, a bias; outputs of 260 storage rows x (N + 8) columns"""

    def __init__(self, L, N, K):
        g = torch.Generator(device="cpu").manual_seed(1000 * N + K)
        self.N, self.K, self.ra, self.rc, self.ldc = N, K, 210, 260, N + 8
        a = (torch.rand((self.ra, K), generator=g) * 2 - 1).cuda()
        b = (torch.rand((N, K), generator=g) * 2 - 1).cuda()
        self.A, self.B = split_rows(L, a, 256.0), split_rows(L, b, 512.0)
        self.descale = 1.0 / (256.0 * 512.0)
        self.bias = (torch.rand(N, generator=g) - 0.5).cuda()
        self.perm_a = torch.randperm(self.ra, generator=g).numpy().astype(np.int32)
        self.perm_c = torch.randperm(self.rc, generator=g).numpy().astype(np.int32)

    def launch(self, L, bound, a_rows, c_rows, count, bias, want_forms):
        """one launch with static row bound `bound` into a sentinel-filled buffer -> the whole buffer"""
        assert L.jlm_gemm_nt_split_form(bound, self.N) in want_forms, (bound, self.N, L.jlm_gemm_nt_split_form(bound, self.N))
        C = torch.full((self.rc, self.ldc), SENTINEL, dtype=torch.float32, device="cuda")
        ar = torch.as_tensor(a_rows, device="cuda") if a_rows is not None else None
        cr = torch.as_tensor(c_rows, device="cuda") if c_rows is not None else None
        nd = torch.tensor([count], dtype=torch.int32, device="cuda") if count is not None else None
        rc = L.jlm_gemm_nt_split(self.A.data_ptr(), self.K, ar.data_ptr() if ar is not None else None, self.B.data_ptr(), self.K, None,
                                 C.data_ptr(), self.ldc, cr.data_ptr() if cr is not None else None,
                                 self.bias.data_ptr() if bias else None, float(self.descale), bound, self.N, self.K,
                                 nd.data_ptr() if nd is not None else None, _st())
        assert rc == 0
        torch.cuda.synchronize()
        return C.cpu().numpy()

    def both(self, L, M, a_rows, c_rows, count=None, bias=True):
        """the ring kernel at bound M (maps may be None: identity) and the tile kernel at the oracle's bound with the same first M rows"""
        got = self.launch(L, M, a_rows, c_rows, count, bias, (JLM_T_SPLIT3_LINEAR, JLM_T_SPLIT3_XCD))
        big = oracle_bound(self.N)
        pad = np.full(big - M, -1, np.int32)
        a_big = np.concatenate([np.arange(M, dtype=np.int32) if a_rows is None else a_rows, pad])
        c_big = np.concatenate([np.arange(M, dtype=np.int32) if c_rows is None else c_rows, pad])
        want = self.launch(L, big, a_big, c_big, count, bias, (JLM_T_CFG64,))
        return got, want


def written_rows(M, c_rows, count):
    n = M if count is None else min(count, M)
    return (np.arange(n) if c_rows is None else c_rows[:n]).astype(np.int64)


def check(P, got, want, M, c_rows, count=None):
    assert got.tobytes() == want.tobytes(), (M, P.N, P.K, count, np.argwhere(got != want)[:4])
    rows = written_rows(M, c_rows, count)
    mask = np.ones(P.rc, bool)
    mask[rows] = False
    assert (got[mask] == SENTINEL).all() and (got[:, P.N:] == SENTINEL).all()      # untouched rows and the padding columns
    assert (got[rows, :P.N] != SENTINEL).all()


def test_oracle_bounds():
    """no GPU: the bounds the oracle launches use (2 752 at the decode's N, as the form's rule gives it)"""
    assert [oracle_bound(N) for N in (40, 256, 352)] == [16448, 4160, 2752]


@gpu
@pytest.mark.parametrize("K", [16, 32, 64, 96, 512])
@pytest.mark.parametrize("N", [40, 256, 352])
def test_ring_equals_tile_kernel(L, N, K):
    P = Problem(L, N, K)
    for M in MS:
        # identity rows, no bias
        got, want = P.both(L, M, None, None, bias=False)
        check(P, got, want, M, None)
        assert np.abs(got[:M, :N]).max() > 0
        # gathered operand rows with a -1 entry (a zero row: its output is the bias), output rows scattered by c_map
        a_rows = P.perm_a[:M].copy()
        a_rows[M // 2] = -1
        c_rows = P.perm_c[:M].copy()
        got, want = P.both(L, M, a_rows, c_rows)
        check(P, got, want, M, c_rows)
        np.testing.assert_array_equal(got[c_rows[M // 2], :N], P.bias.cpu().numpy())
    # device-side counts 0, 1, M under the static bound M
    for M in (65, 200):
        c_rows = P.perm_c[:M].copy()
        for count in (0, 1, M):
            got, want = P.both(L, M, P.perm_a[:M].copy(), c_rows, count=count)
            check(P, got, want, M, c_rows, count)
            if count == 0:
                assert (got == SENTINEL).all()
