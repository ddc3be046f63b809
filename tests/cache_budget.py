"""The derived error bar of cache_rows_kernel (csrc/jlm_cache.hip), shared by tests/test_gpu_cache_rows.py -- whose docstring holds the
derivation, term by term -- and tests/test_gpu_cache.py.  Nothing here is measured: every figure follows from the arithmetic the
kernel uses (the matrix pipe's accumulation bound of DESIGN.md 4.0, one f32 rounding per operation, expf / logf within an ulp)."""
import numpy as np

U = 2.0 ** -24


def e_products(split, H):
    """relative to A = sum_k |q_k| |k_k|: the error of one product h_q . h_i off the matrix pipe"""
    return (3 * H / 16) * 2.0 ** -22 * (1 + 2.0 ** -9) + 2.0 ** -22 if split else H * U / (1 - H * U)


def e_sums(N):
    """relative error of each of the two f32 online sums of at most N positive terms"""
    tiles = -(-(N + 62) // 32)
    stages = 2 * -(-tiles // 16)
    return (2 + N + 3 * (stages + 2)) * U * 1.01


def kernel_bar(split, H, N, theta, A, logM, logZ):
    """BAR_q of tests/test_gpu_cache_rows.py: A = the largest sum_k |q_k| |k_k| over the window, logM / logZ the reference's two
    logarithms under the running maximum"""
    ds = float(np.float32(theta)) * A * (e_products(split, H) + 4 * U)
    return 2 * ds + 2 * e_sums(N) + 2 * U * (abs(logM) + abs(logZ) + 1) + U * abs(logM - logZ)
