"""A NumPy restatement of the greedy max-min selection (``inducing_points``, ``gh_inducing_select``), and the seeded data the
selection tests share.

``maxmin(x, m, first)``: ``idx[0] = first`` and ``dmin = +inf``; for j = 1, 2, ...: ``dmin = min(dmin, d2(x, x[idx[j-1]]))``,
then ``idx[j]`` = the index of the largest ``dmin``, the lower index among equals; after the last pick ``dmin`` is updated once
more.  ``d2`` is accumulated one column at a time, left to right (``s = s + d * d``), one rounding per operation: that is the
device's sum in ANY dimension, and for up to 7 columns also NumPy's ``((x - c)**2).sum(axis=1)``.
"""
import functools

import numpy as np

KINDS = ["1d_unsorted", "2d", "3d", "5d", "7d", "lattice", "clusters", "const_col", "all_equal"]
KINDS_MANY_DIMS = ["9d", "16d", "lattice9"]                 # the device against this file only, never against the host route


def d2_left_to_right(x, c):
    s = np.zeros(len(x))
    for k in range(x.shape[1]):
        d = x[:, k] - c[k]
        s = s + d * d
    return s


def maxmin(x, m, first):
    """``(idx, dmin)``: ``min(m, N)`` int64 indices in the order chosen, and every point's squared distance to the chosen set"""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    k = min(int(m), n)
    idx = np.empty(k, dtype=np.int64)
    dmin = np.full(n, np.inf)
    if n == 0:
        return idx, dmin
    idx[0] = first
    for j in range(1, k + 1):
        dmin = np.minimum(dmin, d2_left_to_right(x, x[idx[j - 1]]))
        if j < k:
            idx[j] = np.argmax(dmin)                        # (the first of equals: the lower index)
    return idx, dmin


def centroid_first(x):
    """the host rule for the first point: nearest the centroid"""
    return int(np.argmin(((x - x.mean(axis=0)) ** 2).sum(axis=1)))


@functools.lru_cache(maxsize=None)
def data(kind, n=1500):
    rng = np.random.RandomState(sum(map(ord, kind)) + n)
    if kind == "1d_unsorted":
        x = rng.uniform(0, 10, (n, 1))
    elif kind == "lattice":                                 # 144 distinct points: exact ties, and repeats past 144 picks
        x = rng.randint(0, 12, (n, 2)).astype(np.float64)
    elif kind == "lattice9":
        x = rng.randint(0, 4, (n, 9)).astype(np.float64)
    elif kind == "clusters":                                # two tight clusters 100 apart
        x = 1e-3 * rng.randn(n, 2)
        x[n // 2:] += 100.0
        x = x[rng.permutation(n)]
    elif kind == "const_col":
        x = rng.uniform(0, 1, (n, 3))
        x[:, 1] = 0.25
    elif kind == "all_equal":
        x = np.tile(rng.uniform(0, 1, (1, 2)), (n, 1))
    else:
        x = rng.uniform(0, 1, (n, int(kind[:-1])))
    x = np.ascontiguousarray(x)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def reference(kind, m, n=1500, first=None):
    """``maxmin`` of ``data(kind, n)`` from the centroid rule's first point (or ``first``), computed once and read-only"""
    x = data(kind, n)
    idx, dmin = maxmin(x, m, centroid_first(x) if first is None else first)
    idx.setflags(write=False)
    dmin.setflags(write=False)
    return idx, dmin
