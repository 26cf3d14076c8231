"""Spectral response functions of instrument channels sampled on a uniform wavenumber grid w_i = w0 + i dw, i < n, in the
form api.make_channels takes: (first, weights_per_channel, centers).  Pure numpy."""
import numpy as np


def _clip(w0, dw, n, lo, hi, what):
    """The grid indices i_lo .. i_hi (inclusive) with lo <= w_i <= hi, clipped to 0 .. n - 1; none: ValueError."""
    eps = 1e-9                                   # (a limit that is a grid point up to rounding takes that point)
    i_lo = max(int(np.ceil((lo - w0) / dw - eps)), 0)
    i_hi = min(int(np.floor((hi - w0) / dw + eps)), n - 1)
    if i_hi < i_lo:
        raise ValueError(f"{what} [{lo}, {hi}] cm-1 has no point on the grid {w0} + i {dw}, i < {n}")
    return i_lo, i_hi


def gaussian(w0, dw, n, centers, fwhm, cutoff_fwhm=4.0):
    """Gaussian channels exp(-4 ln 2 ((w - centre)/fwhm)^2) about each of `centers` (cm-1), cut off at cutoff_fwhm x fwhm
    on either side and clipped to the grid.  fwhm: one value or one per channel.  A channel with no point on the grid
    raises ValueError."""
    centers = np.atleast_1d(np.asarray(centers, dtype=np.float64))
    widths = np.broadcast_to(np.asarray(fwhm, dtype=np.float64), centers.shape)
    first, weights = [], []
    for c, f in zip(centers, widths):
        i_lo, i_hi = _clip(w0, dw, n, c - cutoff_fwhm * f, c + cutoff_fwhm * f, f"the Gaussian channel at {c}")
        w = w0 + np.arange(i_lo, i_hi + 1) * dw
        first.append(i_lo)
        weights.append(np.exp(-4.0 * np.log(2.0) * ((w - c) / f) ** 2))
    return np.array(first, dtype=np.int32), weights, centers.copy()


def boxcar(w0, dw, n, lo, hi):
    """Boxcar channels: weight 1 at every grid point in [lo[c], hi[c]] cm-1, clipped to the grid; the centres are the
    midpoints of the limits as given.  A channel with no point on the grid raises ValueError."""
    lo = np.atleast_1d(np.asarray(lo, dtype=np.float64))
    hi = np.atleast_1d(np.asarray(hi, dtype=np.float64))
    first, weights = [], []
    for a, b in zip(lo, hi):
        i_lo, i_hi = _clip(w0, dw, n, a, b, "the boxcar channel")
        first.append(i_lo)
        weights.append(np.ones(i_hi - i_lo + 1))
    return np.array(first, dtype=np.int32), weights, 0.5 * (lo + hi)
