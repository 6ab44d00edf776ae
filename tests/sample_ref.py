"""Shared by tests/test_sample_host.py and tests/test_gpu_sample.py: the inputs and the two derived bounds of the sampling tests
(their derivation is in the docstring of test_sample_host.py)."""
import numpy as np

EPS = np.finfo(np.float64).eps


def default_tol(a):
    return len(a) * EPS * max(np.max(np.diagonal(a)), 0.0)


def check_factor(a, L, piv, rank, tol):
    """The properties every factor has: reconstruction bound, triangularity in pivot order, zero columns past the rank."""
    m = len(a)
    assert 0 <= rank <= m
    err = np.max(np.abs(a - L @ L.T))
    assert err <= 2 * tol, (err, tol)
    assert np.all(L[:, rank:] == 0.0)
    p = piv[:rank]
    assert len(set(p.tolist())) == rank and np.all((p >= 0) & (p < m))
    assert np.all(np.triu(L[p][:, :rank], 1) == 0.0)                 # L[piv[i], j] == 0 exactly for i < j
    assert np.all(np.diagonal(L[p][:, :rank]) > 0)
    return err


def affine_law(draws, mean, z, fac, rank, m):
    want = mean + z[:, :rank] @ fac[:, :rank].T
    bound = 8 * m * EPS * (np.abs(z[:, :rank]) @ np.abs(fac[:, :rank]).T + np.abs(mean))
    assert np.all(np.abs(draws - want) <= bound), np.max(np.abs(draws - want) / np.maximum(bound, 1e-300))


def low_rank(m, k):
    g = np.random.default_rng(3).standard_normal((m, k))
    return g @ g.T
