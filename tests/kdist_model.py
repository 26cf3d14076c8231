"""The k-distribution reduction of grt_ext.h (grt_kdist_rows) in numpy, for the tests: per bin and class the number of the
bin's points in the class, the sum of their trapezoid weights and the sum of weight x tau.  The classes come from plain
comparisons, the sums from np.cumsum, which adds in index order: what the device must reproduce bit for bit."""
import numpy as np


def classes(tau, class_edges):
    """the number of class edges <= tau, per point: NaN and everything below the first edge 0, +inf the last class"""
    with np.errstate(invalid="ignore"):
        return (np.asarray(class_edges)[None, :] <= np.asarray(tau)[:, None]).sum(1)


def sequential_sum(terms):
    """the left-to-right sum from +0.0"""
    return np.cumsum(np.concatenate(([0.0], terms)))[-1]


def kdist_row(tau, dw, edges, class_edges, weight=None):
    """One row tau [n] -> points (int32), weight, tau, each [num_bins][K]."""
    tau = np.asarray(tau, dtype=np.float64)
    class_edges = np.asarray(class_edges, dtype=np.float64)
    K, nb = class_edges.size + 1, len(edges) - 1
    points = np.zeros((nb, K), dtype=np.int32)
    wsum, tsum = np.zeros((nb, K)), np.zeros((nb, K))
    for b in range(nb):
        lo, hi = int(edges[b]), int(edges[b + 1])
        x = tau[lo:hi + 1]
        w = np.full(x.size, float(dw))
        w[0] = w[-1] = 0.5 * dw
        W = w if weight is None else w * np.asarray(weight, dtype=np.float64)[lo:hi + 1]
        with np.errstate(invalid="ignore", over="ignore"):
            T = W * x
        cls = classes(x, class_edges)
        for k in np.unique(cls):           # (the classes that hold no point keep their zeros)
            sel = cls == k
            points[b, k] = np.count_nonzero(sel)
            with np.errstate(invalid="ignore", over="ignore"):
                wsum[b, k] = sequential_sum(W[sel])
                tsum[b, k] = sequential_sum(T[sel])
    return points, wsum, tsum


def kdist_rows(tau, dw, edges, class_edges, weight=None):
    """Rows tau [rows][n] -> points, weight, tau, each [rows][num_bins][K]."""
    out = [kdist_row(r, dw, edges, class_edges, weight) for r in np.asarray(tau, dtype=np.float64)]
    return tuple(np.array([o[i] for o in out]) for i in range(3))


def same_bits(a, b):
    """two arrays of doubles, equal bit for bit"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))
