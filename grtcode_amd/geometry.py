"""Geometry of the direct beam on a spherical planet, for the layer cosines of api.make_zenith_slant."""
import ctypes as C

import numpy as np

from . import api

EARTH_RADIUS = 6.371e6      # m
RD = 287.05                 # J kg-1 K-1, dry air
G0 = 9.80665                # m s-2


def slant_cosines(radius, heights, mu):
    """grt_slant_cosines: the cosine, in every layer, of the straight ray that reaches the column's lowest level under mu.
    radius: the planet's, m (0: a flat planet -- every layer gets mu itself); heights [ncol][V] m, top first, strictly
    descending; mu [ncol][Z].  Returns [ncol][Z][V - 1], top layer first; an angle below the horizon (mu < 0) gets zeros.
    Raises api.GrtError for what the C function refuses."""
    h = np.ascontiguousarray(heights, dtype=np.float64)
    m = np.ascontiguousarray(mu, dtype=np.float64)
    if h.ndim != 2 or m.ndim != 2 or h.shape[0] != m.shape[0]:
        raise ValueError(f"heights of shape {h.shape} and mu of shape {m.shape}: [ncol][V] and [ncol][Z]")
    ncol, V = h.shape
    Z = m.shape[1]
    out = np.empty((ncol, Z, max(V - 1, 0)), dtype=np.float64)
    dp = C.POINTER(C.c_double)
    api.check(api.load_library().grt_slant_cosines(C.c_double(radius), ncol, V, Z, h.ctypes.data_as(dp), m.ctypes.data_as(dp),
                                                   out.ctypes.data_as(dp)))
    return out


def level_heights(p, t_layer, surface_height=0.0):
    """Hypsometric heights of the levels of pressure p [..][V] (any unit, top first, > 0) over layers of temperature
    t_layer [..][V - 1] K: dz = RD T_layer / G0 ln(p_bottom / p_top), summed up from surface_height (m) at the lowest
    level.  Returns [..][V] m, top first."""
    p = np.asarray(p, dtype=np.float64)
    t = np.asarray(t_layer, dtype=np.float64)
    if np.any(~(p > 0.0)):
        raise ValueError("pressure <= 0 (or NaN): the hypsometric equation takes its logarithm")
    dz = RD * t / G0 * np.log(p[..., 1:] / p[..., :-1])
    z = np.zeros(p.shape, dtype=np.float64)
    z[..., :-1] = np.cumsum(dz[..., ::-1], axis=-1)[..., ::-1]
    return z + surface_height
