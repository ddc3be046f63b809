"""The sample distributions of the k-means compressor's tests (CPU and GPU)."""
import numpy as np


def draw(name, n, seed=1):
    """the issue's six distributions, float32 [n]"""
    rng = np.random.default_rng(seed)
    if name == "gauss":
        x = rng.normal(0, 0.05, n)
    elif name == "t3":
        x = 0.05 * rng.standard_t(3, n)
    elif name == "uniform":
        x = rng.uniform(-1, 1, n)
    elif name == "bimodal":
        x = np.where(rng.random(n) < 0.5, rng.normal(-0.3, 0.02, n), rng.normal(0.2, 0.1, n))
    elif name == "laplace":
        x = rng.laplace(0, 0.05, n)
    elif name == "t2":
        x = 0.05 * rng.standard_t(2, n)
    else:
        raise ValueError(name)
    return x.astype(np.float32)
