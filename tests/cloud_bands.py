"""Band-level cloud optics for the batched pipeline's all-sky pass, restated in numpy for tests (beside cloud_model.py,
whose pieces it reuses): the per-band optics grt_clouds_band_optics returns, the band-limit array framework/src/driver.c
passes to cloud_optics as "wavenumbers" (driver.c:476-488), and the band each grid point takes under spread()'s rules."""
import numpy as np

from cloud_model import beta_lookup, ice_size, pade, spread


def band_optics(tables, rand, cf, lwc, iwc, overlap, liquid_radius, temperature):
    """-> liquid [3][B][L], ice [3][B][L] (extinction, albedo, asymmetry), B = the liquid tables' band count: the draws and
    values of cloud_model.cloud_optics, not spread."""
    L = cf.size
    B = tables["liquid"]["Band_limits_lwr"].size
    liquid, ice = np.zeros((3, B, L)), np.zeros((3, B, L))
    beta = tables["beta"]
    p = q = 5
    for band in range(B):
        rank = np.array([rand() for _ in range(L)])
        decide = np.array([rand() for _ in range(L - 1)])
        for i in range(L - 1):
            if decide[i] <= overlap[i]:
                rank[i + 1] = rank[i]
        for i in range(L):
            ql = qi = 0.0
            if rank[i] > 1.0 - cf[i]:
                qs = beta_lookup(beta, beta["inverse"], p, q, 1.0 - cf[i])
                width = (lwc[i] + iwc[i]) / ((p / (p + q)) * (1.0 - beta_lookup(beta, beta["data"], p + 1, q, qs)) - qs * cf[i])
                total = width * (beta_lookup(beta, beta["inverse"], p, q, rank[i]) - qs)
                frac = lwc[i] / (lwc[i] + iwc[i])
                ql, qi = total * frac, total * (1.0 - frac)
            liquid[:, band, i] = pade(tables["liquid"], ql, liquid_radius, band)
            ice[:, band, i] = pade(tables["ice"], qi, ice_size(temperature[i]) / 2.0, band)
    return liquid, ice


def spread_bands(tables, liquid, ice, w, out=None):
    """band_optics' arrays onto the points w as cloud_optics spreads them: six [L][n] arrays (liquid, then ice)."""
    B, L = liquid.shape[1], liquid.shape[2]
    out = [np.zeros((L, w.size)) for _ in range(6)] if out is None else out
    for band in range(B):
        for i in range(L):
            spread(tables["liquid"], band, w, liquid[:, band, i], [a[i] for a in out[:3]])
            spread(tables["ice"], band, w, ice[:, band, i], [a[i] for a in out[3:]])
    return out


def driver_limits(w0, dw, n):
    """The n values driver.c:476-488 hands to cloud_optics for a grid of n points from w0 by dw: band limits."""
    centres = w0 + np.arange(n, dtype=np.uint64).astype(np.float64) * dw
    w = np.empty(n)
    w[1:] = 0.5 * (centres[:-1] + centres[1:])
    w[0] = max(centres[0] - dw, 0.0)
    return w


def band_map(lo, hi, own_bands, num_bands, w):
    """The band each point of w ends up with when bands 0 .. num_bands - 1 are spread in order (-1: none), for a
    parametrisation of own_bands bands with limits lo / hi."""
    idx = -np.ones(w.size, dtype=np.int64)
    rows = [idx]
    t = {"Band_limits_lwr": np.asarray(lo, dtype=np.float64)[:own_bands], "Band_limits_upr": np.asarray(hi, dtype=np.float64)[:own_bands]}
    for band in range(num_bands):
        spread(t, band, w, [band], rows)
    return idx


def grid_optics(liquid, ice, thickness, maps):
    """Pipeline semantics on one band's grid: [L][n] tau, omega, g of liquid and of ice; tau = extinction x layer
    thickness; no cloud where a point has no band."""
    out = []
    for phase, m in ((liquid, maps[0]), (ice, maps[1])):
        L, n = phase.shape[2], m.size
        vals = [np.zeros((L, n)) for _ in range(3)]
        has = m >= 0
        for k in range(3):
            vals[k][:, has] = phase[k][m[has]].T
        vals[0] = vals[0] * thickness[:, None]
        out += vals
    return out
