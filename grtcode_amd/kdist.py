"""From the device's k-distribution sums (Pipeline.run_kdist / kdist, api.kdist_rows; grt_ext.h: grt_kdist_rows) to the
tables a correlated-k scheme holds: g at the class edges and the mean optical depth of g-intervals.  Pure numpy, no GPU.

The device gives, per (row, bin) and class k of ascending optical depth, `weight` -- the sum of the trapezoid weights
(times the spectral weight) of the bin's points in the class -- and `tau`, the sum of weight x optical depth.  The classes
lie along the last axis of both arrays; every function works on that axis and keeps the others.
"""
import numpy as np


def cumulative(weight):
    """g at the upper edge of every class: cumsum(weight) / sum(weight) along the last axis, so g[..., -1] == 1.  A bin
    whose weights are all zero gives NaN."""
    w = np.asarray(weight, dtype=np.float64)
    total = w.sum(axis=-1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.cumsum(w, axis=-1) / total


def k_of_g(weight, tau, g_edges):
    """The mean optical depth of each interval g_edges[j] .. g_edges[j + 1] of the cumulative probability g: [..., G] for
    G + 1 ascending g_edges in 0 .. 1.  Within a class the optical depth counts as its class mean tau/weight over the
    class's whole width in g, so a class that a g-edge cuts is split in proportion to its weight; the means of contiguous
    intervals, weighted with their widths, add up to sum(tau)/sum(weight).  A bin whose weights are all zero gives NaN."""
    w = np.asarray(weight, dtype=np.float64)
    t = np.asarray(tau, dtype=np.float64)
    ge = np.asarray(g_edges, dtype=np.float64).ravel()
    if w.shape != t.shape:
        raise ValueError(f"weight {w.shape} and tau {t.shape} differ in shape")
    if ge.size < 2 or np.any(np.diff(ge) <= 0.0) or ge[0] < 0.0 or ge[-1] > 1.0:
        raise ValueError("g_edges: at least two, strictly increasing, in 0 .. 1")
    K = w.shape[-1]
    w2, t2 = w.reshape(-1, K), t.reshape(-1, K)
    out = np.full((w2.shape[0], ge.size - 1), np.nan)
    for r in range(w2.shape[0]):
        total = w2[r].sum()
        if not total > 0.0:
            continue
        # the integral of the optical depth over 0 .. g: piecewise linear through the class edges
        g = np.concatenate(([0.0], np.cumsum(w2[r]) / total))
        integral = np.concatenate(([0.0], np.cumsum(t2[r]) / total))
        at = np.interp(ge, g, integral)
        out[r] = np.diff(at) / np.diff(ge)
    return out.reshape(w.shape[:-1] + (ge.size - 1,))


def correlated_k_of_g(weight, tau, g_edges):
    """k_of_g for every row of a correlated reduction (Pipeline.run_kdist_correlated, api.kdist_mapped_rows): weight
    [..., bins, K] is shared by the R rows of tau [..., R, bins, K] -- every row was summed over the same classes of points
    -- and is broadcast over the row axis: [..., R, bins, G].  The g-intervals are then the same sets of spectral points in
    every row, which is what makes the rows' k(g) correlated."""
    w = np.asarray(weight, dtype=np.float64)
    t = np.asarray(tau, dtype=np.float64)
    if t.ndim != w.ndim + 1 or t.ndim < 3 or t.shape[:-3] != w.shape[:-2] or t.shape[-2:] != w.shape[-2:]:
        raise ValueError(f"weight {w.shape} is not tau {t.shape} without its row axis")
    return k_of_g(np.broadcast_to(w[..., None, :, :], t.shape), t, g_edges)


def ck_means(weight, tau, source):
    """The class means a correlated-k flux solve works on (Pipeline.run_ck_fluxes / ck_fluxes; grt_ext.h:
    grt_pipeline_run_ck_fluxes): weight [..., bins, K] -> (tau_mean [..., L, bins, K], source_mean [..., R, bins, K]), each
    class sum divided by its class weight, 0 where the weight is 0 (a class of no points, which the solver skips).  The
    longwave's source rows are then the Planck function per cm-1 at the levels, the layers and the surface and the
    emissivity of each g-point; the shortwave's row 1, the solar curve, goes into the solver as its sum, not its mean."""
    w = np.asarray(weight, dtype=np.float64)
    out = []
    for x in (tau, source):
        x = np.asarray(x, dtype=np.float64)
        if x.ndim != w.ndim + 1 or x.ndim < 3 or x.shape[:-3] != w.shape[:-2] or x.shape[-2:] != w.shape[-2:]:
            raise ValueError(f"weight {w.shape} is not {x.shape} without its row axis")
        wb = np.broadcast_to(w[..., None, :, :], x.shape)
        mean = np.zeros(x.shape)
        np.divide(x, wb, out=mean, where=wb > 0.0)
        out.append(mean)
    return tuple(out)
