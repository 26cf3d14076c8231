"""The correlated k-distributions of grt_ext.h (grt_kdist_class_map, grt_kdist_mapped_rows) in numpy, for the tests: the key
of every group, its class map, and the reduction of every row under that map -- the classes by kdist_model.classes, the
sums by kdist_model.sequential_sum: what the device must reproduce bit for bit."""
import numpy as np

from kdist_model import classes, sequential_sum

KEY_ROW, KEY_SUM = 0, 1


def key_rows(x, kind, key_row=0):
    """x [G][R][n] -> the key [G][n]: row key_row of every group, or the rows' sum in order from +0.0, every add rounded"""
    x = np.asarray(x, dtype=np.float64)
    if kind == KEY_ROW:
        return x[:, key_row, :].copy()
    if kind != KEY_SUM:
        raise ValueError(f"key kind {kind}")
    key = np.zeros((x.shape[0], x.shape[2]))
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(x.shape[1]):
            key = key + x[:, r, :]
    return key


def class_map(x, kind, class_edges, key_row=0):
    """x [G][R][n] -> map [G][n], uint16: the class of every group's key at every point"""
    key = key_rows(x, kind, key_row)
    return np.array([classes(row, class_edges) for row in key]).astype(np.uint16)


def mapped_rows(values, map_, dw, edges, K, weight=None):
    """values [G][R][n] under map_ [G][n] -> points (int32) and weight [G][num_bins][K], tau [G][R][num_bins][K].  A map
    entry >= K belongs to no class."""
    values = np.asarray(values, dtype=np.float64)
    map_ = np.asarray(map_)
    G, R, _n = values.shape
    nb = len(edges) - 1
    points = np.zeros((G, nb, K), dtype=np.int32)
    wsum, tsum = np.zeros((G, nb, K)), np.zeros((G, R, nb, K))
    for g in range(G):
        for b in range(nb):
            lo, hi = int(edges[b]), int(edges[b + 1])
            w = np.full(hi - lo + 1, float(dw))
            w[0] = w[-1] = 0.5 * dw
            W = w if weight is None else w * np.asarray(weight, dtype=np.float64)[lo:hi + 1]
            with np.errstate(invalid="ignore", over="ignore"):
                T = W[None, :] * values[g, :, lo:hi + 1]
            cls = map_[g, lo:hi + 1].astype(np.int64)
            for k in np.unique(cls):
                if k >= K:
                    continue
                sel = cls == k
                points[g, b, k] = np.count_nonzero(sel)
                wsum[g, b, k] = sequential_sum(W[sel])
                for r in range(R):
                    with np.errstate(invalid="ignore", over="ignore"):
                        tsum[g, r, b, k] = sequential_sum(T[r, sel])
    return points, wsum, tsum
