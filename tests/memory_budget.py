"""The derived error bar of memory_rows_kernel / memory_fold_kernel (csrc/jlm_memory.hip), shared by tests/test_gpu_memory_rows.py --
whose docstring holds the derivation, term by term -- and tests/test_gpu_memory.py.  Nothing here is measured: the products' term is
cache_rows_kernel's (tests/cache_budget.py e_products: the same instructions in the same order), the sums' term is restated for this
kernel's own count of rescale stages."""
import numpy as np

from tests.cache_budget import U, e_products

MIN_SPLIT_KEYS = 512
MAX_SPLITS = 128


def keys_per_split(N):
    """S of include/jlm_hip.h: max(512, ceil(ceil(N / 128) / 64) * 64)"""
    return max(MIN_SPLIT_KEYS, -(-(-(-N // MAX_SPLITS)) // 64) * 64)


def rescale_stages(N):
    """the most stages a partial sum passes: a wave's tile stages within one split -- ceil(min(S, N) / 32) tiles in pairs, wave w taking
    the pairs w, w + 8, ..., two tile stages a pair -- then the half-wave fold, the eight-wave fold and the split fold"""
    tiles = -(-min(keys_per_split(N), N) // 32)
    pairs = -(-tiles // 2)
    return 2 * -(-pairs // 8) + 3


def e_sums(N):
    """relative error of each of the two f32 online sums of N positive terms"""
    return (2 + N + 3 * rescale_stages(N)) * U * 1.01


def kernel_bar(split, H, N, theta, A, logM, logZ):
    """BAR_q of tests/test_gpu_memory_rows.py: A = the largest sum_k |q_k| |k_k| over the memory, logM / logZ the reference's two
    logarithms under the running maximum"""
    ds = float(np.float32(theta)) * A * (e_products(split, H) + 4 * U)
    return 2 * ds + 2 * e_sums(N) + 2 * U * (abs(logM) + abs(logZ) + 1) + U * abs(logM - logZ)
