"""Spectral response functions of level fluxes sampled on a uniform wavenumber grid w_i = w0 + i dw, i < n, in the form
api.make_responses takes for a band: (first, weights_list) -- the grid index of each response's first point and its
values from that point on.  The values are NOT normalised: Pipeline.run_sky_weighted returns sum_i t_i r(i) F_i, t_i the
trapezoid weight.  Pure numpy."""
import numpy as np

from .channels import _clip

PLANCK = 6.62607015e-34          # J s
LIGHT_SPEED = 299792458.0        # m s-1
AVOGADRO = 6.02214076e23         # mol-1
PAR_LIMITS = (14285.7, 25000.0)  # cm-1: 700 nm .. 400 nm


def join(*responses):
    """Several (first, weights_list) of one band as one."""
    first = np.concatenate([np.atleast_1d(np.asarray(f, dtype=np.int32)) for f, _ in responses])
    return first, [np.asarray(w, dtype=np.float64) for _, ws in responses for w in ws]


def tabulated(w0, dw, n, x, y, unit="cm-1"):
    """One response from a table: y at the knots x (strictly increasing, in cm-1 or -- unit="nm" -- in nm, wavelength =
    1e7 / wavenumber), linear IN THE GIVEN UNIT between the knots, zero outside them, clipped to the grid.  No grid point
    inside the table: ValueError."""
    x = np.asarray(x, dtype=np.float64).ravel()
    y = np.asarray(y, dtype=np.float64).ravel()
    if unit not in ("cm-1", "nm"):
        raise ValueError(f"unit {unit!r}: 'cm-1' or 'nm'")
    if x.size < 2 or x.size != y.size or np.any(np.diff(x) <= 0):
        raise ValueError("the table needs two or more strictly increasing knots, and a value at each")
    lo, hi = (x[0], x[-1]) if unit == "cm-1" else (1e7 / x[-1], 1e7 / x[0])
    i_lo, i_hi = _clip(w0, dw, n, lo, hi, "the tabulated response")
    w = w0 + np.arange(i_lo, i_hi + 1) * dw
    at = np.clip(w if unit == "cm-1" else 1e7 / w, x[0], x[-1])      # (an end point that is a knot up to rounding)
    return np.array([i_lo], dtype=np.int32), [np.interp(at, x, y)]


def band(w0, dw, n, lo, hi):
    """One response that is 1 at every grid point in [lo, hi] cm-1, clipped to the grid.  None: ValueError."""
    i_lo, i_hi = _clip(w0, dw, n, lo, hi, "the band")
    return np.array([i_lo], dtype=np.int32), [np.ones(i_hi - i_lo + 1)]


def photon_weight_at(wavenumber):
    """Micromoles of photons per joule at `wavenumber` (cm-1): 1e6 / (N_A h c nu)."""
    nu = np.asarray(wavenumber, dtype=np.float64) * 100.0            # m-1
    return 1e6 / (AVOGADRO * PLANCK * LIGHT_SPEED * nu)


def photon_weight(w0, dw, n, lo=PAR_LIMITS[0], hi=PAR_LIMITS[1]):
    """One response that turns W m-2 into umol photons m-2 s-1 over [lo, hi] cm-1 (default: photosynthetically active
    radiation, 400 - 700 nm): photon_weight_at(w_i) inside, 0 outside, clipped to the grid.  None: ValueError."""
    i_lo, i_hi = _clip(w0, dw, n, lo, hi, "the photon-weighted band")
    return np.array([i_lo], dtype=np.int32), [photon_weight_at(w0 + np.arange(i_lo, i_hi + 1) * dw)]


def erythemal_action(wavelength_nm):
    """The CIE erythemal action spectrum (ISO/CIE 17166) at `wavelength_nm`: 1 for 250 <= l <= 298, 10^(0.094 (298 - l)) up
    to 328, 10^(0.015 (140 - l)) up to 400, 0 elsewhere."""
    lam = np.asarray(wavelength_nm, dtype=np.float64)
    out = np.zeros(lam.shape)
    flat = (lam >= 250.0) & (lam <= 298.0)
    mid = (lam > 298.0) & (lam <= 328.0)
    far = (lam > 328.0) & (lam <= 400.0)
    out[flat] = 1.0
    out[mid] = 10.0 ** (0.094 * (298.0 - lam[mid]))
    out[far] = 10.0 ** (0.015 * (140.0 - lam[far]))
    return out


def erythemal(w0, dw, n):
    """One response: the erythemal action spectrum at l = 1e7 / w_i nm over the grid's points in 250 .. 400 nm (25 000 ..
    40 000 cm-1).  The UV index is 40 m2 W-1 x the weighted downward flux at the surface.  None: ValueError."""
    i_lo, i_hi = _clip(w0, dw, n, 1e7 / 400.0, 1e7 / 250.0, "the erythemal action spectrum")
    lam = 1e7 / (w0 + np.arange(i_lo, i_hi + 1) * dw)
    return np.array([i_lo], dtype=np.int32), [erythemal_action(np.clip(lam, 250.0, 400.0))]
