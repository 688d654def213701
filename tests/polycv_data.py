"""Inputs and oracles shared by test_polycv_cpu.py and test_polycv_gpu.py."""
import numpy as np
import torch

from bodywork_mlops_demo_amd.ops import reference

DEFAULT_L2_GRID = (0.0, 1e-6, 1e-4, 1e-2, 1.0)


def integer_rows(n, seed=0):
    """x in {-3..3}, y in {-8..8} as fp32: with mu=0, s=1 every statistic
    is an integer far inside 2^53, so fp64 sums are exact in any order."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-3, 4, n)
    y = rng.integers(-8, 9, n)
    return x, y


def int64_fold_stats(x, y, folds, seed=42, ids=None):
    """[folds, 18] int64: S_0..S_10, T_0..T_5, Q per fold (``ids``: the
    rows' folds when the caller already holds them)."""
    if ids is None:
        ids = reference.fold_ids_cpu(len(x), folds, seed)
    x = x.astype(np.int64)
    y = y.astype(np.int64)
    out = np.zeros((folds, 18), dtype=np.int64)
    for f in range(folds):
        xf, yf = x[ids == f], y[ids == f]
        for p in range(11):
            out[f, p] = (xf ** p).sum()
        for q in range(6):
            out[f, 11 + q] = (yf * xf ** q).sum()
        out[f, 17] = (yf * yf).sum()
    return out


def as_f32(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float32))


def quadratic_rows(n=4099):
    """y = 3 + 2t - 4t^2 + 0.5 N(0,1), t = (x-50)/50, x ~ U(0,100)."""
    rng = np.random.default_rng(20261021)
    x = rng.uniform(0, 100, n)
    t = (x - 50.0) / 50.0
    y = 3.0 + 2.0 * t - 4.0 * t * t + 0.5 * rng.standard_normal(n)
    return as_f32(x), as_f32(y)
